// Pooling and resampling for gfx950: max-pool forward / backward (argmax
// codes, deterministic gather), bilinear interpolation and its backward,
// per-image pixel sums and their broadcast.
// Entries: include/upr_train.h; layout and precision: train_common.h.
#include <cmath>

#include "train_common.h"

namespace upr {

// ---------------------------------------------------------------------------
// pooling / resampling
// ---------------------------------------------------------------------------
__global__ void maxpool_kernel(V x, int B, int H, int W, int C, int k, int s, int p, V y, int Ho, int Wo) {
  const long long n = (long long)B * Ho * Wo * C;
  GSTRIDE(i, n) {
    const int c = (int)(i % C);
    long long r = i / C;
    const int ox = (int)(r % Wo); r /= Wo;
    const int oy = (int)(r % Ho);
    const int b = (int)(r / Ho);
    float m = -INFINITY;
    for (int ky = 0; ky < k; ++ky) {
      const int iy = oy * s - p + ky;
      if (iy < 0 || iy >= H) continue;
      for (int kx = 0; kx < k; ++kx) {
        const int ix = ox * s - p + kx;
        if (ix < 0 || ix >= W) continue;
        const float v = x.d[x.at(b, iy, ix, c)];
        if (v > m || isnan(v)) m = v;
      }
    }
    y.d[y.at(b, oy, ox, c)] = m;
  }
}

// Max-pool backward as two deterministic passes (no float atomics):
//  1. per output element the window position of its max, PyTorch's rule
//     (max_pool2d CPU kernel: the first in-bounds tap, then every tap with
//     v > max or v NaN), as a byte code ky * k + kx;
//  2. per input element, in output order, the dy of every window whose code
//     points at it, added to dx.
template <int VEC>
__global__ void maxpool_arg_kernel(V x, int B, int H, int W, int C, int k, int s, int p, int Ho, int Wo,
                                   unsigned char* __restrict__ code) {
  const int CV = C / VEC;
  const long long n = (long long)B * Ho * Wo * CV;
  GSTRIDE(i, n) {
    const int c = (int)(i % CV) * VEC;
    long long r = i / CV;
    const int ox = (int)(r % Wo); r /= Wo;
    const int oy = (int)(r % Ho);
    const int b = (int)(r / Ho);
    float m[VEC];
    int best[VEC];
#pragma unroll
    for (int v = 0; v < VEC; ++v) { m[v] = -INFINITY; best[v] = -1; }
    for (int ky = 0; ky < k; ++ky) {
      const int iy = oy * s - p + ky;
      if (iy < 0 || iy >= H) continue;
      for (int kx = 0; kx < k; ++kx) {
        const int ix = ox * s - p + kx;
        if (ix < 0 || ix >= W) continue;
        float val[VEC];
        if constexpr (VEC == 4) {
          const float4 q = *(const float4*)(x.d + x.at(b, iy, ix, c));
          val[0] = q.x; val[1] = q.y; val[2] = q.z; val[3] = q.w;
        } else {
          val[0] = x.d[x.at(b, iy, ix, c)];
        }
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
          if (best[v] < 0) best[v] = ky * k + kx;  // the first in-bounds tap is the default index
          if (val[v] > m[v] || isnan(val[v])) {
            m[v] = val[v];
            best[v] = ky * k + kx;
          }
        }
      }
    }
    unsigned char* o = code + (((long long)b * Ho + oy) * Wo + ox) * C + c;
#pragma unroll
    for (int v = 0; v < VEC; ++v) o[v] = (unsigned char)(best[v] < 0 ? 255 : best[v]);
  }
}

template <int VEC>
__global__ void maxpool_bwd_gather_kernel(const unsigned char* __restrict__ code, V dy, int B, int H, int W, int C, int k,
                                          int s, int p, int Ho, int Wo, V dx) {
  const int CV = C / VEC;
  const long long n = (long long)B * H * W * CV;
  GSTRIDE(i, n) {
    const int c = (int)(i % CV) * VEC;
    long long r = i / CV;
    const int ix = (int)(r % W); r /= W;
    const int iy = (int)(r % H);
    const int b = (int)(r / H);
    float* dp = dx.d + dx.at(b, iy, ix, c);
    float acc[VEC];
    if constexpr (VEC == 4) {
      const float4 q = *(const float4*)dp;
      acc[0] = q.x; acc[1] = q.y; acc[2] = q.z; acc[3] = q.w;
    } else {
      acc[0] = *dp;
    }
    // windows containing (iy, ix): oy*s - p <= iy <= oy*s - p + k - 1
    const int oy0 = max(0, (iy + p - k + 1 + s - 1 + s * k) / s - k), oy1 = min(Ho - 1, (iy + p) / s);
    const int ox0 = max(0, (ix + p - k + 1 + s - 1 + s * k) / s - k), ox1 = min(Wo - 1, (ix + p) / s);
    for (int oy = oy0; oy <= oy1; ++oy) {
      const int ty = iy - (oy * s - p);
      if (ty < 0 || ty >= k) continue;
      for (int ox = ox0; ox <= ox1; ++ox) {
        const int tx = ix - (ox * s - p);
        if (tx < 0 || tx >= k) continue;
        const unsigned char want = (unsigned char)(ty * k + tx);
        const unsigned char* cd = code + (((long long)b * Ho + oy) * Wo + ox) * C + c;
        const float* g = dy.d + dy.at(b, oy, ox, c);
#pragma unroll
        for (int v = 0; v < VEC; ++v)
          if (cd[v] == want) acc[v] += g[v * dy.sc];
      }
    }
    if constexpr (VEC == 4) {
      *(float4*)dp = make_float4(acc[0], acc[1], acc[2], acc[3]);
    } else {
      *dp = acc[0];
    }
  }
}

// Fast paths for the two pools of the training step -- EnhancedFAM's 3x3/1/1
// (models/model.py:32) and the VGG 2x2/2 (losses/loss.py perceptual
// features[4], [9], [18]) -- on channel-contiguous views: 4 channels per
// thread, 32-bit index math (the generic kernels' 64-bit div/mod per element
// ran at <1 TB/s), compile-time windows.  The forward optionally writes the
// argmax byte codes (PyTorch's rule, as maxpool_arg_kernel) so the backward
// is the gather alone.
// TI = half_t: the input is an activation's compact fp16 copy (the autocast
// VGG activations live in fp16 only, as the reference's under autocast)
template <int K, int S, int P, typename TI = float>
__global__ __launch_bounds__(256) void maxpool4_kernel(const TI* __restrict__ x, int xsb, int xsh, int xsw, int H,
                                                       int W, int CV, int Ho, int Wo, int n, float* __restrict__ y,
                                                       int ysb, int ysh, int ysw, unsigned* __restrict__ code,
                                                       half_t* __restrict__ y16) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int c = (i % CV) * 4;
  int r = i / CV;
  const int ox = r % Wo;
  r /= Wo;
  const int oy = r % Ho, b = r / Ho;
  float m[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
  int best[4] = {-1, -1, -1, -1};
  const TI* xb = x + b * xsb + c;
#pragma unroll
  for (int ky = 0; ky < K; ++ky) {
    const int iy = oy * S - P + ky;
    if ((unsigned)iy >= (unsigned)H) continue;
#pragma unroll
    for (int kx = 0; kx < K; ++kx) {
      const int ix = ox * S - P + kx;
      if ((unsigned)ix >= (unsigned)W) continue;
      const float4 q = ld4f(xb + iy * xsh + ix * xsw);
      const float val[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        if (best[v] < 0) best[v] = ky * K + kx;
        if (val[v] > m[v] || isnan(val[v])) {
          m[v] = val[v];
          best[v] = ky * K + kx;
        }
      }
    }
  }
  if (y) *(float4*)(y + b * ysb + oy * ysh + ox * ysw + c) = make_float4(m[0], m[1], m[2], m[3]);
  if (y16) {  // compact [b][oy][ox][C] fp16 copy: element index 4 i
    typedef _Float16 h4 __attribute__((ext_vector_type(4)));
    *(h4*)(y16 + (size_t)i * 4) = h4{(half_t)m[0], (half_t)m[1], (half_t)m[2], (half_t)m[3]};
  }
  if (code) {
    unsigned w = 0;
#pragma unroll
    for (int v = 0; v < 4; ++v) w |= (unsigned)(best[v] < 0 ? 255 : best[v]) << (8 * v);
    code[i] = w;
  }
}

// dx[b][iy][ix][c..c+3] += dy of every window (ascending oy, then ox: the
// generic gather's order) whose code points at (iy, ix).  O16: the result
// goes to the compact fp16 g16 instead (element 4 i), masked by the producing
// ReLU's fp16 output y16 when given -- the frozen VGG's pool backward, whose
// only reader is the masked fp16 dgrad operand (relu_mask16h fused away)
template <int K, int S, int P, int O16 = 0>
__global__ __launch_bounds__(256) void maxpool_gather4_kernel(const unsigned* __restrict__ code,
                                                              const float* __restrict__ dy, int dsb, int dsh, int dsw,
                                                              int H, int W, int CV, int Ho, int Wo, int n,
                                                              float* __restrict__ dx, int xsb, int xsh, int xsw,
                                                              int accumulate, const half_t* __restrict__ y16 = nullptr,
                                                              half_t* __restrict__ g16 = nullptr) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int cv = i % CV, c = cv * 4;
  int r = i / CV;
  const int ix = r % W;
  r /= W;
  const int iy = r % H, b = r / H;
  float* dp = O16 ? nullptr : dx + b * xsb + iy * xsh + ix * xsw + c;
  float4 acc = !O16 && accumulate ? *(const float4*)dp : make_float4(0.f, 0.f, 0.f, 0.f);
  // every window's code word and gradient run is loaded first (independent
  // loads, one round trip each; a window outside the output reads nothing and
  // gets the no-hit code 0xffffffff), then the hits are added in the same
  // window order as before (the 3x3 pool's code -> dy -> next window chain
  // was 18 dependent round trips per thread: 1.6 TB/s at 512^2)
  unsigned wv[K * K];
  float4 gv[K * K];
#pragma unroll
  for (int t = 0; t < K; ++t) {
    const int ky = K - 1 - t, ny = iy + P - ky;  // oy * S
    const bool oky = ny >= 0 && ny % S == 0 && ny / S < Ho;
    const int oy = oky ? ny / S : 0;
#pragma unroll
    for (int u = 0; u < K; ++u) {
      const int kx = K - 1 - u, nx = ix + P - kx;
      const bool ok = oky && nx >= 0 && nx % S == 0 && nx / S < Wo;
      const int ox = ok ? nx / S : 0;
      wv[t * K + u] = ok ? code[((b * Ho + oy) * Wo + ox) * CV + cv] : 0xffffffffu;
      gv[t * K + u] = ok ? *(const float4*)(dy + b * dsb + oy * dsh + ox * dsw + c) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
  }
#pragma unroll
  for (int t = 0; t < K; ++t) {
    const int ky = K - 1 - t;
#pragma unroll
    for (int u = 0; u < K; ++u) {
      const int kx = K - 1 - u;
      const unsigned want = (unsigned)(ky * K + kx) * 0x01010101u;
      const unsigned hit = wv[t * K + u] ^ want;  // a zero byte marks a window whose max sits here
      const float4 g = gv[t * K + u];
      if ((hit & 0xffu) == 0) acc.x += g.x;
      if ((hit & 0xff00u) == 0) acc.y += g.y;
      if ((hit & 0xff0000u) == 0) acc.z += g.z;
      if ((hit & 0xff000000u) == 0) acc.w += g.w;
    }
  }
  if (O16) {
    typedef _Float16 h4 __attribute__((ext_vector_type(4)));
    if (y16) {
      const h4 y = *(const h4*)(y16 + (size_t)i * 4);
      if (!(y[0] > (half_t)0)) acc.x = 0.f;
      if (!(y[1] > (half_t)0)) acc.y = 0.f;
      if (!(y[2] > (half_t)0)) acc.z = 0.f;
      if (!(y[3] > (half_t)0)) acc.w = 0.f;
    }
    *(h4*)(g16 + (size_t)i * 4) = h4{(half_t)acc.x, (half_t)acc.y, (half_t)acc.z, (half_t)acc.w};
    return;
  }
  *(float4*)dp = acc;
}

__global__ void zero_view_kernel(V v, int B, int H, int W, int C) {
  const long long n = (long long)B * H * W * C;
  GSTRIDE(i, n) {
    const int c = (int)(i % C);
    long long r = i / C;
    const int x = (int)(r % W);
    r /= W;
    v.d[v.at((int)(r / H), (int)(r % H), x, c)] = 0.f;
  }
}

// shape of a fast-path pool: (k, s, p) one of the two instantiated windows,
// channel-contiguous 16-byte aligned views whose extents fit 32-bit offsets
static int pool_fast_kind(int k, int s, int p) {
  if (k == 3 && s == 1 && p == 1) return 1;
  if (k == 2 && s == 2 && p == 0) return 2;
  return 0;
}

__device__ __forceinline__ void bilin_src(int o, int in, float scale, int& i0, int& i1, float& l) {
  float sr = ((float)o + 0.5f) * scale - 0.5f;
  if (sr < 0.f) sr = 0.f;
  i0 = (int)sr;
  if (i0 > in - 1) i0 = in - 1;
  i1 = i0 + (i0 < in - 1 ? 1 : 0);
  l = sr - (float)i0;
}

__global__ void bilinear_kernel(V x, int B, int H, int W, int C, V y, int Ho, int Wo, float sh, float sw, int accum) {
  const long long n = (long long)B * Ho * Wo * C;
  GSTRIDE(i, n) {
    const int c = (int)(i % C);
    long long r = i / C;
    const int ox = (int)(r % Wo); r /= Wo;
    const int oy = (int)(r % Ho);
    const int b = (int)(r / Ho);
    int y0, y1, x0, x1;
    float ly, lx;
    bilin_src(oy, H, sh, y0, y1, ly);
    bilin_src(ox, W, sw, x0, x1, lx);
    const float v = (1.f - ly) * ((1.f - lx) * x.d[x.at(b, y0, x0, c)] + lx * x.d[x.at(b, y0, x1, c)]) +
                    ly * ((1.f - lx) * x.d[x.at(b, y1, x0, c)] + lx * x.d[x.at(b, y1, x1, c)]);
    float* o = y.d + y.at(b, oy, ox, c);
    *o = accum ? *o + v : v;
  }
}

// gather form of the bilinear backward: one thread per SOURCE element sums the
// output gradients whose forward taps (bilin_src, the forward's own arithmetic)
// land on it -- no atomics (the scatter form contends 16-256 ways on the 4x /
// 16x head upsamplings).  Candidate outputs: those whose source coordinate lies
// in [i-1, i+1]; the last row / column also collects the clamped tail.
__device__ __forceinline__ void bilin_range(int i, int in, int out, float scale, int& lo, int& hi) {
  lo = (int)floorf(((float)i - 0.5f) / scale - 0.5f) - 1;
  hi = (int)ceilf(((float)i + 1.5f) / scale - 0.5f) + 1;
  if (lo < 0) lo = 0;
  if (i == in - 1 || hi > out - 1) hi = out - 1;
}

__device__ __forceinline__ float bilin_w(int o, int i, int in, float scale) {
  int i0, i1;
  float l;
  bilin_src(o, in, scale, i0, i1, l);
  return (i0 == i ? 1.f - l : 0.f) + (i1 == i ? l : 0.f);
}

__global__ void bilinear_bwd_gather_kernel(V dy, int B, int H, int W, int C, int Ho, int Wo, float sh, float sw, V dx) {
  const long long n = (long long)B * H * W * C;
  GSTRIDE(i, n) {
    const int c = (int)(i % C);
    long long r = i / C;
    const int ix = (int)(r % W); r /= W;
    const int iy = (int)(r % H);
    const int b = (int)(r / H);
    int ylo, yhi, xlo, xhi;
    bilin_range(iy, H, Ho, sh, ylo, yhi);
    bilin_range(ix, W, Wo, sw, xlo, xhi);
    float acc = 0.f;
    for (int oy = ylo; oy <= yhi; ++oy) {
      const float wy = bilin_w(oy, iy, H, sh);
      if (wy == 0.f) continue;
      float row = 0.f;
      for (int ox = xlo; ox <= xhi; ++ox) {
        const float wx = bilin_w(ox, ix, W, sw);
        if (wx != 0.f) row += wx * dy.d[dy.at(b, oy, ox, c)];
      }
      acc += wy * row;
    }
    dx.d[dx.at(b, iy, ix, c)] += acc;
  }
}

// 4-channel forms (V4 views, one thread per pixel and 4 channels)
__global__ __launch_bounds__(256) void bilinear4_kernel(V4 x, int H, int W, int CV, V4 y, int Ho, int Wo, float sh,
                                                        float sw, int n, int accum, half_t* __restrict__ y16,
                                                        int cs16) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  int b, oy, ox, c;
  dec4(i, CV, Wo, Ho, b, oy, ox, c);
  int y0, y1, x0, x1;
  float ly, lx;
  bilin_src(oy, H, sh, y0, y1, ly);
  bilin_src(ox, W, sw, x0, x1, lx);
  const float4 a = *(const float4*)x.at(b, y0, x0, c), bq = *(const float4*)x.at(b, y0, x1, c);
  const float4 cq = *(const float4*)x.at(b, y1, x0, c), d = *(const float4*)x.at(b, y1, x1, c);
  // the scalar kernel's expression per channel
  float4 v;
  v.x = (1.f - ly) * ((1.f - lx) * a.x + lx * bq.x) + ly * ((1.f - lx) * cq.x + lx * d.x);
  v.y = (1.f - ly) * ((1.f - lx) * a.y + lx * bq.y) + ly * ((1.f - lx) * cq.y + lx * d.y);
  v.z = (1.f - ly) * ((1.f - lx) * a.z + lx * bq.z) + ly * ((1.f - lx) * cq.z + lx * d.z);
  v.w = (1.f - ly) * ((1.f - lx) * a.w + lx * bq.w) + ly * ((1.f - lx) * cq.w + lx * d.w);
  float4* o = (float4*)y.at(b, oy, ox, c);
  if (accum == 1) {
    const float4 u = *o;
    v = make_float4(u.x + v.x, u.y + v.y, u.z + v.z, u.w + v.w);
  }
  if (accum != 2) *o = v;  // 2: the fp16 copy only
  if (y16) store16(y16, cs16, i / CV, c, v);
}

// bilinear backward, separable and in the gather kernel's summation order:
// pass 1 row[b][oy][ix] = sum over ox (ascending, nonzero weights) of
// wx * dy[b][oy][ox]; pass 2 dx[b][iy][ix] += sum over oy (ascending, nonzero
// weights) of wy * row[b][oy][ix].  Each pass scans ~3/scale candidates
// instead of the product of both axes.
__global__ __launch_bounds__(256) void bilinear_bwd_rows4_kernel(V4 dy, int Ho, int Wo, int W, int CV, float sw,
                                                                 float* __restrict__ row, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  int b, oy, ix, c;
  dec4(i, CV, W, Ho, b, oy, ix, c);
  int xlo, xhi;
  bilin_range(ix, W, Wo, sw, xlo, xhi);
  float4 r = make_float4(0.f, 0.f, 0.f, 0.f);
  // four taps' loads issued together per pass (the tap loop of one load per
  // dependent step ran the 4x / 16x upsample backward at ~3 TB/s); zero-weight
  // taps are skipped as before, so the sums are unchanged
  for (int ox0 = xlo; ox0 <= xhi; ox0 += 4) {
    float wx[4];
    float4 g[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int ox = ox0 + k;
      wx[k] = ox <= xhi ? bilin_w(ox, ix, W, sw) : 0.f;
      g[k] = wx[k] != 0.f ? *(const float4*)dy.at(b, oy, ox, c) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (wx[k] == 0.f) continue;
      r.x += wx[k] * g[k].x;
      r.y += wx[k] * g[k].y;
      r.z += wx[k] * g[k].z;
      r.w += wx[k] * g[k].w;
    }
  }
  *(float4*)(row + (size_t)i * 4) = r;
}

__global__ __launch_bounds__(256) void bilinear_bwd_cols4_kernel(const float* __restrict__ row, int Ho, int H, int W,
                                                                 int CV, float sh, V4 dx, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  int b, iy, ix, c;
  dec4(i, CV, W, H, b, iy, ix, c);
  int ylo, yhi;
  bilin_range(iy, H, Ho, sh, ylo, yhi);
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  const int C = CV * 4;
  for (int oy = ylo; oy <= yhi; ++oy) {
    const float wy = bilin_w(oy, iy, H, sh);
    if (wy == 0.f) continue;
    const float4 r = *(const float4*)(row + (((size_t)b * Ho + oy) * W + ix) * C + c);
    acc.x += wy * r.x;
    acc.y += wy * r.y;
    acc.z += wy * r.z;
    acc.w += wy * r.w;
  }
  float4* o = (float4*)dx.at(b, iy, ix, c);
  const float4 u = *o;
  *o = make_float4(u.x + acc.x, u.y + acc.y, u.z + acc.z, u.w + acc.w);
}

// per-(image, channel) pixel sums: grid (chunks, B)
__global__ __launch_bounds__(256) void pixel_sum_kernel(const float* __restrict__ x, int HW, int C, int cs, int coff,
                                                        float scale, float* __restrict__ out) {
  __shared__ float sm[256];
  const int b = blockIdx.y;
  const int per = (HW + gridDim.x - 1) / gridDim.x;
  const int p0 = blockIdx.x * per, p1 = min(HW, p0 + per);
  for (int cb = 0; cb < C; cb += 256) {
    const int cw = min(256, C - cb);
    const int R = 256 / cw;
    const int c = threadIdx.x % cw, rg = threadIdx.x / cw;
    float u = 0.f;
    if (rg < R)
      for (int q = p0 + rg; q < p1; q += R) u += x[((size_t)b * HW + q) * cs + coff + cb + c];
    sm[threadIdx.x] = u;
    __syncthreads();
    if (threadIdx.x < cw) {
      float t = 0.f;
      for (int k = 0; k < R; ++k) t += sm[k * cw + threadIdx.x];
      atomicAdd(out + (size_t)b * C + cb + threadIdx.x, t * scale);
    }
    __syncthreads();
  }
}

// The same with 4 channels per lane (C % 4 == 0, 16-byte rows; C <= 1024) and
// 4 rows of loads in flight per lane, each block's sums stored to its own
// partial slot and added in chunk order by pixel_sum_fin_kernel (the FAM
// pool's 32-channel sum at 512^2 ran at 1.3 TB/s as one float per lane per
// dependent step, and its per-block atomics made the order run-dependent)
__global__ __launch_bounds__(256) void pixel_sum4_kernel(const float* __restrict__ x, int HW, int C, int cs, int coff,
                                                         float* __restrict__ part) {
  __shared__ float4 sm[256];
  const int b = blockIdx.y;
  const int C4 = C >> 2, R = 256 / C4;
  const int per = (HW + gridDim.x - 1) / gridDim.x;
  const int p0 = blockIdx.x * per, p1 = min(HW, p0 + per);
  const int c4 = threadIdx.x % C4, rg = threadIdx.x / C4;
  float4 u = make_float4(0.f, 0.f, 0.f, 0.f);
  if (rg < R) {
    const float* base = x + (size_t)b * HW * cs + coff + 4 * c4;
    int q = p0 + rg;
    for (; q + 3 * R < p1; q += 4 * R) {
      float4 v[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) v[k] = *(const float4*)(base + (size_t)(q + k * R) * cs);
#pragma unroll
      for (int k = 0; k < 4; ++k) { u.x += v[k].x; u.y += v[k].y; u.z += v[k].z; u.w += v[k].w; }
    }
    for (; q < p1; q += R) {
      const float4 v = *(const float4*)(base + (size_t)q * cs);
      u.x += v.x; u.y += v.y; u.z += v.z; u.w += v.w;
    }
  }
  sm[threadIdx.x] = u;
  __syncthreads();
  if (threadIdx.x < C4) {
    float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int k = 0; k < R; ++k) {
      const float4 w = sm[k * C4 + threadIdx.x];
      t.x += w.x; t.y += w.y; t.z += w.z; t.w += w.w;
    }
    *(float4*)(part + ((size_t)b * gridDim.x + blockIdx.x) * C + 4 * threadIdx.x) = t;
  }
}

// out[b][c] (+)= scale * (partials of chunks 0, 1, ... in order)
__global__ __launch_bounds__(256) void pixel_sum_fin_kernel(const float* __restrict__ part, int chunks, int BC, int C,
                                                            float scale, float* __restrict__ out, int accumulate) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= BC) return;
  const int b = j / C, c = j - b * C;
  const float* p = part + (size_t)b * chunks * C + c;
  float t = 0.f;
  int k = 0;
  for (; k + 3 < chunks; k += 4) {
    const float v0 = p[(size_t)k * C], v1 = p[(size_t)(k + 1) * C], v2 = p[(size_t)(k + 2) * C], v3 = p[(size_t)(k + 3) * C];
    t += v0; t += v1; t += v2; t += v3;
  }
  for (; k < chunks; ++k) t += p[(size_t)k * C];
  out[j] = (accumulate ? out[j] : 0.f) + t * scale;
}

// the fp16 form: y16[b][p][coff + c] = (half)(v[b][c] * scale), 4 channels per thread
__global__ void broadcast16_kernel(const float* __restrict__ v, int B, int HW, int C, float scale,
                                   half_t* __restrict__ y16, int y_cs, int y_coff) {
  const int C4 = C / 4;
  const long long n = (long long)B * HW * C4;
  GSTRIDE(i, n) {
    const int c = (int)(i % C4) * 4;
    const long long m = i / C4;
    const int b = (int)(m / HW);
    typedef _Float16 h4 __attribute__((ext_vector_type(4)));
    const float* s = v + (size_t)b * C + c;
    *(h4*)(y16 + m * y_cs + y_coff + c) =
        h4{(half_t)(s[0] * scale), (half_t)(s[1] * scale), (half_t)(s[2] * scale), (half_t)(s[3] * scale)};
  }
}

__global__ void broadcast_kernel(const float* __restrict__ v, int B, int HW, int C, float scale, float* y, int y_cs,
                                 int y_coff, int accum) {
  const long long n = (long long)B * HW * C;
  GSTRIDE(i, n) {
    const int c = (int)(i % C);
    const long long m = i / C;
    const int b = (int)(m / HW);
    float* o = y + m * y_cs + y_coff + c;
    const float val = v[(size_t)b * C + c] * scale;
    *o = accum ? *o + val : val;
  }
}

}  // namespace upr

using namespace upr;

extern "C" {

int upr_t_maxpool(const UprView* x, int B, int H, int W, int C, int k, int s, int p, const UprView* y, int Ho, int Wo,
                  void* stream) {
  return upr_t_maxpool_code(x, B, H, W, C, k, s, p, y, Ho, Wo, nullptr, nullptr, stream);
}

int upr_t_maxpool_bwd(const UprView* x, const UprView* dy, int B, int H, int W, int C, int k, int s, int p, int Ho,
                      int Wo, const UprView* dx, void* stream) {
  if (!x || !dy || !dx || k <= 0 || s <= 0 || k * k > 255) return UPR_ERR_ARG;
  hipStream_t st = ST(stream);
  const long long n = (long long)B * Ho * Wo * C;
  void* code = nullptr;
  code = scratch(kSlotCode, (size_t)n, st);
  if (!code) return (int)hipErrorOutOfMemory;
  const bool v4 = C % 4 == 0 && x->sc == 1 && dx->sc == 1 && (uintptr_t)x->data % 16 == 0 &&
                  (uintptr_t)dx->data % 16 == 0 && x->sw % 4 == 0 && x->sh % 4 == 0 && x->sb % 4 == 0 &&
                  dx->sw % 4 == 0 && dx->sh % 4 == 0 && dx->sb % 4 == 0;
  const long long ni = (long long)B * H * W * C;
  if (v4) {
    hipLaunchKernelGGL(maxpool_arg_kernel<4>, dim3(grid_for(n / 4)), dim3(256), 0, st, mkv(x), B, H, W, C, k, s, p, Ho,
                       Wo, (unsigned char*)code);
    hipLaunchKernelGGL(maxpool_bwd_gather_kernel<4>, dim3(grid_for(ni / 4)), dim3(256), 0, st,
                       (const unsigned char*)code, mkv(dy), B, H, W, C, k, s, p, Ho, Wo, mkv(dx));
  } else {
    hipLaunchKernelGGL(maxpool_arg_kernel<1>, dim3(grid_for(n)), dim3(256), 0, st, mkv(x), B, H, W, C, k, s, p, Ho, Wo,
                       (unsigned char*)code);
    hipLaunchKernelGGL(maxpool_bwd_gather_kernel<1>, dim3(grid_for(ni)), dim3(256), 0, st, (const unsigned char*)code,
                       mkv(dy), B, H, W, C, k, s, p, Ho, Wo, mkv(dx));
  }
  UPR_CHECK_HIP(hipGetLastError());
  return UPR_OK;
}

int upr_t_maxpool_code(const UprView* x, int B, int H, int W, int C, int k, int s, int p, const UprView* y, int Ho,
                       int Wo, unsigned char* code, void* y16, void* stream) {
  if (!x || !y || k <= 0 || s <= 0 || k * k > 255) return UPR_ERR_ARG;
  hipStream_t st = ST(stream);
  const long long n = (long long)B * Ho * Wo * C;
  if (n == 0) return UPR_OK;
  const int kind = pool_fast_kind(k, s, p);
  if (kind && vec4_view_ok(x, B, H, W, C) && vec4_view_ok(y, B, Ho, Wo, C) && (uintptr_t)code % 4 == 0 &&
      (uintptr_t)y16 % 8 == 0 && n < (1LL << 31)) {
    const int nv = (int)(n / 4), CV = C / 4;
    auto go = [&](auto kern) {
      hipLaunchKernelGGL(kern, dim3((nv + 255) / 256), dim3(256), 0, st, (const float*)x->data, (int)x->sb,
                         (int)x->sh, (int)x->sw, H, W, CV, Ho, Wo, nv, (float*)y->data, (int)y->sb, (int)y->sh,
                         (int)y->sw, (unsigned*)code, (half_t*)y16);
    };
    if (kind == 1) go(maxpool4_kernel<3, 1, 1>);
    else go(maxpool4_kernel<2, 2, 0>);
    LAUNCH_CHECK();
  }
  if (y16) return UPR_ERR_UNSUPPORTED;  // the fp16 copy comes with the 4-channel path only
  hipLaunchKernelGGL(maxpool_kernel, dim3(grid_for(n)), dim3(256), 0, st, mkv(x), B, H, W, C, k, s, p, mkv(y), Ho, Wo);
  if (code)
    hipLaunchKernelGGL(maxpool_arg_kernel<1>, dim3(grid_for(n)), dim3(256), 0, st, mkv(x), B, H, W, C, k, s, p, Ho,
                       Wo, code);
  LAUNCH_CHECK();
}

int upr_t_maxpool16_code(const void* x16, int B, int H, int W, int C, int k, int s, int p, const UprView* y, int Ho,
                         int Wo, unsigned char* code, void* y16, void* stream) {
  if (!x16 || !y || k <= 0 || s <= 0 || k * k > 255) return UPR_ERR_ARG;
  if (!y->data && !y16) return UPR_ERR_ARG;  // y->data NULL: the fp16 copy only (its values are exact)
  const long long n = (long long)B * Ho * Wo * C;
  if (n == 0) return UPR_OK;
  const int kind = pool_fast_kind(k, s, p);
  if (!kind || C % 4 || (uintptr_t)x16 % 8 || !vec4_view_ok(y, B, Ho, Wo, C) || (uintptr_t)code % 4 ||
      (uintptr_t)y16 % 8 || (long long)B * H * W * C >= (1LL << 31))
    return UPR_ERR_UNSUPPORTED;
  const int nv = (int)(n / 4), CV = C / 4;
  auto go = [&](auto kern) {
    hipLaunchKernelGGL(kern, dim3((nv + 255) / 256), dim3(256), 0, ST(stream), (const half_t*)x16, H * W * C, W * C,
                       C, H, W, CV, Ho, Wo, nv, (float*)y->data, (int)y->sb, (int)y->sh, (int)y->sw, (unsigned*)code,
                       (half_t*)y16);
  };
  if (kind == 1) go(maxpool4_kernel<3, 1, 1, half_t>);
  else go(maxpool4_kernel<2, 2, 0, half_t>);
  LAUNCH_CHECK();
}

int upr_t_maxpool_bwd_code(const unsigned char* code, const UprView* dy, int B, int H, int W, int C, int k, int s,
                           int p, int Ho, int Wo, const UprView* dx, int accumulate, void* stream) {
  if (!code || !dy || !dx || k <= 0 || s <= 0 || k * k > 255) return UPR_ERR_ARG;
  hipStream_t st = ST(stream);
  const long long ni = (long long)B * H * W * C;
  if (ni == 0) return UPR_OK;
  const int kind = pool_fast_kind(k, s, p);
  if (kind && vec4_view_ok(dy, B, Ho, Wo, C) && vec4_view_ok(dx, B, H, W, C) && (uintptr_t)code % 4 == 0 &&
      ni < (1LL << 31)) {
    const int nv = (int)(ni / 4), CV = C / 4;
    auto go = [&](auto kern) {
      hipLaunchKernelGGL(kern, dim3((nv + 255) / 256), dim3(256), 0, st, (const unsigned*)code,
                         (const float*)dy->data, (int)dy->sb, (int)dy->sh, (int)dy->sw, H, W, CV, Ho, Wo, nv,
                         (float*)dx->data, (int)dx->sb, (int)dx->sh, (int)dx->sw, accumulate, (const half_t*)nullptr,
                         (half_t*)nullptr);
    };
    if (kind == 1) go(maxpool_gather4_kernel<3, 1, 1>);
    else go(maxpool_gather4_kernel<2, 2, 0>);
    LAUNCH_CHECK();
  }
  if (!accumulate) {
    // the generic gather adds into dx: clear the view first
    hipLaunchKernelGGL(zero_view_kernel, dim3(grid_for(ni)), dim3(256), 0, st, mkv(dx), B, H, W, C);
  }
  hipLaunchKernelGGL(maxpool_bwd_gather_kernel<1>, dim3(grid_for(ni)), dim3(256), 0, st, code, mkv(dy), B, H, W, C,
                     k, s, p, Ho, Wo, mkv(dx));
  LAUNCH_CHECK();
}

int upr_t_maxpool_bwd_code16(const unsigned char* code, const UprView* dy, int B, int H, int W, int C, int k, int s,
                             int p, int Ho, int Wo, const void* y16, void* g16, void* stream) {
  if (!code || !dy || !g16 || k <= 0 || s <= 0 || k * k > 255) return UPR_ERR_ARG;
  const long long ni = (long long)B * H * W * C;
  if (ni == 0) return UPR_OK;
  const int kind = pool_fast_kind(k, s, p);
  if (!kind || !vec4_view_ok(dy, B, Ho, Wo, C) || (uintptr_t)code % 4 || (uintptr_t)g16 % 8 || (uintptr_t)y16 % 8 ||
      ni >= (1LL << 31))
    return UPR_ERR_UNSUPPORTED;
  const int nv = (int)(ni / 4), CV = C / 4;
  auto go = [&](auto kern) {
    hipLaunchKernelGGL(kern, dim3((nv + 255) / 256), dim3(256), 0, ST(stream), (const unsigned*)code,
                       (const float*)dy->data, (int)dy->sb, (int)dy->sh, (int)dy->sw, H, W, CV, Ho, Wo, nv,
                       (float*)nullptr, 0, 0, 0, 0, (const half_t*)y16, (half_t*)g16);
  };
  if (kind == 1) go(maxpool_gather4_kernel<3, 1, 1, 1>);
  else go(maxpool_gather4_kernel<2, 2, 0, 1>);
  LAUNCH_CHECK();
}

int upr_t_bilinear(const UprView* x, int B, int H, int W, int C, const UprView* y, int Ho, int Wo, int accumulate,
                   void* stream) {
  if (!x || !y || Ho <= 0 || Wo <= 0) return UPR_ERR_ARG;
  const long long n = (long long)B * Ho * Wo * C;
  if (n == 0) return UPR_OK;
  if (vec4_view_ok(x, B, H, W, C) && vec4_view_ok(y, B, Ho, Wo, C)) {
    const int nv = (int)(n / 4);
    hipLaunchKernelGGL(bilinear4_kernel, dim3((nv + 255) / 256), dim3(256), 0, ST(stream), mkv4(x), H, W, C / 4,
                       mkv4(y), Ho, Wo, (float)H / Ho, (float)W / Wo, nv, accumulate, (half_t*)nullptr, 0);
    LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(bilinear_kernel, dim3(grid_for(n)), dim3(256), 0, ST(stream), mkv(x), B, H, W, C, mkv(y), Ho, Wo,
                     (float)H / Ho, (float)W / Wo, accumulate);
  LAUNCH_CHECK();
}

int upr_t_bilinear_bwd(const UprView* dy, int B, int H, int W, int C, int Ho, int Wo, const UprView* dx,
                       void* stream) {
  if (!dy || !dx) return UPR_ERR_ARG;
  const long long n = (long long)B * Ho * Wo * C;
  if (n > 0 && vec4_view_ok(dy, B, Ho, Wo, C) && vec4_view_ok(dx, B, H, W, C) &&
             (long long)B * Ho * W * C < (1LL << 31)) {
    hipStream_t st = ST(stream);
    const int nr = B * Ho * W * C / 4, ns = B * H * W * C / 4;
    float* row = nullptr;
    row = (float*)scratch(kSlotRows, sizeof(float) * 4 * (size_t)nr, st);
    if (!row) return (int)hipErrorOutOfMemory;
    hipLaunchKernelGGL(bilinear_bwd_rows4_kernel, dim3((nr + 255) / 256), dim3(256), 0, st, mkv4(dy), Ho, Wo, W, C / 4,
                       (float)W / Wo, row, nr);
    hipLaunchKernelGGL(bilinear_bwd_cols4_kernel, dim3((ns + 255) / 256), dim3(256), 0, st, (const float*)row, Ho, H,
                       W, C / 4, (float)H / Ho, mkv4(dx), ns);
    UPR_CHECK_HIP(hipGetLastError());
    return UPR_OK;
  } else {
    const long long ns = (long long)B * H * W * C;
    hipLaunchKernelGGL(bilinear_bwd_gather_kernel, dim3(grid_for(ns)), dim3(256), 0, ST(stream), mkv(dy), B, H, W, C,
                       Ho, Wo, (float)H / Ho, (float)W / Wo, mkv(dx));
  }
  LAUNCH_CHECK();
}

int upr_t_bilinear16(const UprView* x, int B, int H, int W, int C, const UprView* y, int Ho, int Wo, int accumulate,
                     void* y16, int y16_cs, void* stream) {
  if (!x || !y || !y16 || Ho <= 0 || Wo <= 0 || accumulate < 0 || accumulate > 2) return UPR_ERR_ARG;
  const long long n = (long long)B * Ho * Wo * C;
  if (n == 0) return UPR_OK;
  if (!vec4_view_ok(x, B, H, W, C) || !vec4_view_ok(y, B, Ho, Wo, C) || (uintptr_t)y16 % 8 || y16_cs % 4 ||
      (long long)B * Ho * Wo * y16_cs >= (1LL << 31))
    return UPR_ERR_UNSUPPORTED;
  const int nv = (int)(n / 4);
  hipLaunchKernelGGL(bilinear4_kernel, dim3((nv + 255) / 256), dim3(256), 0, ST(stream), mkv4(x), H, W, C / 4, mkv4(y),
                     Ho, Wo, (float)H / Ho, (float)W / Wo, nv, accumulate, (half_t*)y16, y16_cs);
  LAUNCH_CHECK();
}

int upr_t_pixel_sum(const float* x, int B, int HW, int C, int cs, int coff, float scale, float* out, int accumulate,
                    void* stream) {
  if (!x || !out || B <= 0 || HW <= 0 || C <= 0) return UPR_ERR_ARG;
  if (C % 4 == 0 && C <= 1024 && cs % 4 == 0 && coff % 4 == 0 && ((uintptr_t)x & 15) == 0) {
    hipStream_t st = ST(stream);
    // about 32 rows a lane whatever C (R = 256 / (C / 4) row groups a block; C = 32: HW / 1024).
    // HW / 1024 for every C left a lane of the wide forms (C = 256: R = 4, C = 1024: R = 1) a
    // sequential chain of up to 1024 / R rows, 8 ulp off float64 at 300 rows, on a handful of blocks.
    int chunks = HW / (32 * (256 / (C / 4)));
    chunks = chunks < 1 ? 1 : (chunks > 256 ? 256 : chunks);
    float* part = (float*)scratch(kSlotPart, sizeof(float) * (size_t)B * chunks * C, st);
    if (!part) return (int)hipErrorOutOfMemory;
    hipLaunchKernelGGL(pixel_sum4_kernel, dim3(chunks, B), dim3(256), 0, st, x, HW, C, cs, coff, part);
    UPR_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(pixel_sum_fin_kernel, dim3((B * C + 255) / 256), dim3(256), 0, st, (const float*)part, chunks,
                       B * C, C, scale, out, accumulate);
    LAUNCH_CHECK();
  }
  if (!accumulate) UPR_CHECK_HIP(hipMemsetAsync(out, 0, sizeof(float) * B * C, ST(stream)));
  int chunks = HW / 2048;
  chunks = chunks < 1 ? 1 : (chunks > 256 ? 256 : chunks);
  hipLaunchKernelGGL(pixel_sum_kernel, dim3(chunks, B), dim3(256), 0, ST(stream), x, HW, C, cs, coff, scale, out);
  LAUNCH_CHECK();
}

int upr_t_broadcast(const float* v, int B, int HW, int C, float scale, float* y, int y_cs, int y_coff, int accumulate,
                    void* stream) {
  if (!v || !y || B <= 0 || HW <= 0 || C <= 0 || y_cs < y_coff + C) return UPR_ERR_ARG;
  const long long n = (long long)B * HW * C;
  hipLaunchKernelGGL(broadcast_kernel, dim3(grid_for(n)), dim3(256), 0, ST(stream), v, B, HW, C, scale, y, y_cs,
                     y_coff, accumulate);
  LAUNCH_CHECK();
}

int upr_t_broadcast16(const float* v, int B, int HW, int C, float scale, void* y16, int y_cs, int y_coff,
                      void* stream) {
  if (!v || !y16 || B <= 0 || HW <= 0 || C <= 0 || y_cs < y_coff + C) return UPR_ERR_ARG;
  if (C % 4 || y_cs % 4 || y_coff % 4 || (uintptr_t)y16 % 8) return UPR_ERR_UNSUPPORTED;
  const long long n = (long long)B * HW * (C / 4);
  hipLaunchKernelGGL(broadcast16_kernel, dim3(grid_for(n)), dim3(256), 0, ST(stream), v, B, HW, C, scale,
                     (half_t*)y16, y_cs, y_coff);
  LAUNCH_CHECK();
}

}  // extern "C"
