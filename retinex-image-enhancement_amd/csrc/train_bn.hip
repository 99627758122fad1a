// Per-channel reductions and BatchNorm2d (training and eval statistics,
// apply, backward) for gfx950: two-stage fp64 reductions whose block
// partials are added in a fixed order, with atomic fallbacks.
// Entries: include/upr_train.h; layout and precision: train_common.h.
#include <cmath>

#include "train_common.h"

namespace upr {

// ---------------------------------------------------------------------------
// per-channel reductions over M rows: mode 0 (x, x^2), mode 1 (g, g*xhat),
// mode 2 (g) -> float out via atomics
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void chan_reduce_kernel(const float* __restrict__ a, int a_cs, int a_coff,
                                                          const float* __restrict__ x, int x_cs, int x_coff,
                                                          const float* __restrict__ mean,
                                                          const float* __restrict__ invstd, int M, int C, int mode,
                                                          double* __restrict__ acc, float* __restrict__ fout) {
  __shared__ double s1[256], s2[256];
  const int rows_per_block = (M + gridDim.x - 1) / gridDim.x;
  const int r0 = blockIdx.x * rows_per_block;
  const int r1 = min(M, r0 + rows_per_block);
  for (int cb = 0; cb < C; cb += 256) {
    const int cw = min(256, C - cb);
    const int R = 256 / cw;
    const int c = threadIdx.x % cw, rg = threadIdx.x / cw;
    double u = 0.0, v = 0.0;
    if (rg < R) {
      const int cc = cb + c;
      float mu = 0.f, is = 0.f;
      if (mode == 1) { mu = mean[cc]; is = invstd[cc]; }
      for (int r = r0 + rg; r < r1; r += R) {
        const float av = a[(size_t)r * a_cs + a_coff + cc];
        if (mode == 0) { u += av; v += (double)av * av; }
        else if (mode == 1) { u += av; v += (double)av * ((x[(size_t)r * x_cs + x_coff + cc] - mu) * is); }
        else u += av;
      }
    }
    s1[threadIdx.x] = u;
    s2[threadIdx.x] = v;
    __syncthreads();
    if (threadIdx.x < cw) {
      double t1 = 0.0, t2 = 0.0;
      for (int k = 0; k < R; ++k) { t1 += s1[k * cw + threadIdx.x]; t2 += s2[k * cw + threadIdx.x]; }
      const int cc = cb + threadIdx.x;
      if (mode == 2) atomicAdd(fout + cc, (float)t1);
      else { atomicAdd(acc + cc, t1); atomicAdd(acc + C + cc, t2); }
    }
    __syncthreads();
  }
}

static int reduce_grid(int M) { return grid_for(M, 512, 2048); }

// float4 form of chan_reduce_kernel (C % 4 == 0, C <= 1024, 16-byte aligned
// rows): a thread owns 4 consecutive channels, so a wave reads whole 16-byte
// chunks of 64 / (C/4) rows per instruction (same per-channel fp64 sums)
// y = bn(x) of the forward (bn_apply kernels) and of the ReLU-mask recompute
// in the fused backward: ONE expression, so the recomputed sign is the
// forward's bit for bit
__device__ __forceinline__ float bn_affine(float x, float mean, float invstd, float gamma, float beta) {
  return __builtin_fmaf((x - mean) * invstd, gamma, beta);
}

__global__ __launch_bounds__(256) void chan_reduce4_kernel(const float* __restrict__ a, int a_cs, int a_coff,
                                                           const float* __restrict__ x, int x_cs, int x_coff,
                                                           const float* __restrict__ mean,
                                                           const float* __restrict__ invstd, int M, int C, int mode,
                                                           double* __restrict__ acc, float* __restrict__ fout,
                                                           const float* __restrict__ gamma = nullptr,
                                                           const float* __restrict__ beta = nullptr) {
  // mode 3: mode 1 with the consumer ReLU folded in (g counts where bn(x) > 0)
  __shared__ double s1[256 * 4], s2[256 * 4];
  const int rows_per_block = (M + gridDim.x - 1) / gridDim.x;
  const int r0 = blockIdx.x * rows_per_block;
  const int r1 = min(M, r0 + rows_per_block);
  const int C4 = C >> 2;
  const int R = 256 / C4;
  const int q = threadIdx.x % C4, rg = threadIdx.x / C4;
  double u[4] = {0.0, 0.0, 0.0, 0.0}, v[4] = {0.0, 0.0, 0.0, 0.0};
  if (rg < R) {
    float4 mu = make_float4(0.f, 0.f, 0.f, 0.f), is = mu, ga = mu, be = mu;
    if (mode == 1 || mode == 3) { mu = ((const float4*)mean)[q]; is = ((const float4*)invstd)[q]; }
    if (mode == 3) { ga = ((const float4*)gamma)[q]; be = ((const float4*)beta)[q]; }
    auto acc_row = [&](const float4 av, const float4 xv) {
      float ae[4] = {av.x, av.y, av.z, av.w};
      if (mode == 1 || mode == 3) {
        const float xe[4] = {xv.x, xv.y, xv.z, xv.w};
        const float mue[4] = {mu.x, mu.y, mu.z, mu.w}, ise[4] = {is.x, is.y, is.z, is.w};
        const float gae[4] = {ga.x, ga.y, ga.z, ga.w}, bee[4] = {be.x, be.y, be.z, be.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          if (mode == 3 && !(bn_affine(xe[e], mue[e], ise[e], gae[e], bee[e]) > 0.f)) ae[e] = 0.f;
          const float xh = (xe[e] - mue[e]) * ise[e];
          u[e] += ae[e];
          v[e] += (double)ae[e] * xh;
        }
      } else if (mode == 0) {
#pragma unroll
        for (int e = 0; e < 4; ++e) { u[e] += ae[e]; v[e] += (double)ae[e] * ae[e]; }
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) u[e] += ae[e];
      }
    };
    // four rows' loads issued before any is consumed (a single dependent load
    // per iteration left the reduction latency-bound at ~1.2 TB/s)
    const float* ap = a + a_coff + 4 * q;
    const float* xp = x ? x + x_coff + 4 * q : nullptr;
    int r = r0 + rg;
    for (; r + 3 * R < r1; r += 4 * R) {
      float4 av[4], xv[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) av[k] = *(const float4*)(ap + (size_t)(r + k * R) * a_cs);
      if (mode == 1 || mode == 3) {
#pragma unroll
        for (int k = 0; k < 4; ++k) xv[k] = *(const float4*)(xp + (size_t)(r + k * R) * x_cs);
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) acc_row(av[k], (mode == 1 || mode == 3) ? xv[k] : av[k]);
    }
    for (; r < r1; r += R)
      acc_row(*(const float4*)(ap + (size_t)r * a_cs),
              (mode == 1 || mode == 3) ? *(const float4*)(xp + (size_t)r * x_cs) : make_float4(0.f, 0.f, 0.f, 0.f));
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) { s1[threadIdx.x * 4 + e] = u[e]; s2[threadIdx.x * 4 + e] = v[e]; }
  __syncthreads();
  if (threadIdx.x < C4) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      double t1 = 0.0, t2 = 0.0;
      for (int k = 0; k < R; ++k) { t1 += s1[(k * C4 + threadIdx.x) * 4 + e]; t2 += s2[(k * C4 + threadIdx.x) * 4 + e]; }
      const int cc = 4 * threadIdx.x + e;
      if (mode == 2) atomicAdd(fout + cc, (float)t1);
      else { atomicAdd(acc + cc, t1); atomicAdd(acc + C + cc, t2); }
    }
  }
}

static bool reduce4_ok(int C, int cs, int coff, const void* p) {
  return C % 4 == 0 && C <= 1024 && cs % 4 == 0 && coff % 4 == 0 && ((uintptr_t)p & 15) == 0;
}

// Two-stage per-channel reductions (the float4 path): kRedSlots blocks of 1024
// threads each write their per-channel partial sums to a slot of their own
// (plain stores), then one small kernel adds the slots in slot order.  The
// single-stage form ended every block with 2C same-address fp64 atomics, which
// serialised at the L2 (1.2-1.8 TB/s on the training shapes); this one is also
// deterministic run to run.  Modes as chan_reduce4_kernel (0: x, x^2; 1: g,
// g*xhat; 2: g; 3: mode 1 with the consumer ReLU folded in).
constexpr int kRedSlots = 256;
constexpr int kRedThreads = 1024;

// TA / TX = half_t: the operand is an activation's compact fp16 copy (the
// autocast conv output's exact values: BatchNorm reads half the bytes)
template <typename TA = float, typename TX = float>
__global__ __launch_bounds__(kRedThreads) void chan_part_kernel(const TA* __restrict__ a, int a_cs, int a_coff,
                                                                const TX* __restrict__ x, int x_cs, int x_coff,
                                                                const float* __restrict__ mean,
                                                                const float* __restrict__ invstd,
                                                                const float* __restrict__ gamma,
                                                                const float* __restrict__ beta, int M, int C, int mode,
                                                                double* __restrict__ part) {
  extern __shared__ double red_sm[];  // [R][2C]: R * C = 4096
  const int C4 = C >> 2;
  const int R = kRedThreads / C4;
  const int q = threadIdx.x % C4, rg = threadIdx.x / C4;
  const int rows_per_block = (M + gridDim.x - 1) / gridDim.x;
  const int r0 = blockIdx.x * rows_per_block;
  const int r1 = min(M, r0 + rows_per_block);
  const bool gx = mode == 1 || mode == 3;
  double u[4] = {0.0, 0.0, 0.0, 0.0}, v[4] = {0.0, 0.0, 0.0, 0.0};
  if (rg < R) {
    float mu[4] = {0.f, 0.f, 0.f, 0.f}, is[4] = {0.f, 0.f, 0.f, 0.f}, ga[4] = {0.f, 0.f, 0.f, 0.f},
          be[4] = {0.f, 0.f, 0.f, 0.f};
    if (gx) {
#pragma unroll
      for (int e = 0; e < 4; ++e) { mu[e] = mean[4 * q + e]; is[e] = invstd[4 * q + e]; }
    }
    if (mode == 3) {
#pragma unroll
      for (int e = 0; e < 4; ++e) { ga[e] = gamma[4 * q + e]; be[e] = beta[4 * q + e]; }
    }
    const TA* ap = a + a_coff + 4 * q;
    const TX* xp = x ? x + x_coff + 4 * q : nullptr;
    auto row = [&](const float4 av, const float4 xv) {
      float ae[4] = {av.x, av.y, av.z, av.w};
      const float xe[4] = {xv.x, xv.y, xv.z, xv.w};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        if (gx) {
          if (mode == 3 && !(bn_affine(xe[e], mu[e], is[e], ga[e], be[e]) > 0.f)) ae[e] = 0.f;
          u[e] += ae[e];
          v[e] += (double)ae[e] * ((xe[e] - mu[e]) * is[e]);
        } else if (mode == 0) {
          u[e] += ae[e];
          v[e] += (double)ae[e] * ae[e];
        } else {
          u[e] += ae[e];
        }
      }
    };
    int r = r0 + rg;
    // one-operand modes (the forward statistics): 8 rows' loads in flight per
    // thread (4 left the 512^2 statistics passes latency-bound at ~3 TB/s),
    // then the 4-row batches, then single rows
    if (!gx) {
      for (; r + 7 * R < r1; r += 8 * R) {
        float4 av[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) av[k] = ld4f(ap + (size_t)(r + k * R) * a_cs);
#pragma unroll
        for (int k = 0; k < 8; ++k) row(av[k], av[k]);
      }
    }
    for (; r + 3 * R < r1; r += 4 * R) {
      float4 av[4], xv[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) av[k] = ld4f(ap + (size_t)(r + k * R) * a_cs);
      if (gx) {
#pragma unroll
        for (int k = 0; k < 4; ++k) xv[k] = ld4f(xp + (size_t)(r + k * R) * x_cs);
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) row(av[k], gx ? xv[k] : av[k]);
    }
    for (; r < r1; r += R)
      row(ld4f(ap + (size_t)r * a_cs), gx ? ld4f(xp + (size_t)r * x_cs) : make_float4(0.f, 0.f, 0.f, 0.f));
  }
  if (rg < R) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      red_sm[rg * 2 * C + 4 * q + e] = u[e];
      red_sm[rg * 2 * C + C + 4 * q + e] = v[e];
    }
  }
  __syncthreads();
  double* dst = part + (size_t)blockIdx.x * 2 * C;
  for (int t = threadIdx.x; t < 2 * C; t += kRedThreads) {
    double s = 0.0;
    for (int k = 0; k < R; ++k) s += red_sm[k * 2 * C + t];
    dst[t] = s;
  }
}

// slot sums -> acc[2C] (modes 0/1/3, overwritten) or out[C] (+)= (mode 2), in
// a fixed order: a block owns 64 outputs (one per lane), wave w adds slots
// w, w + 4, ... in that order, 16 loads issued together per batch (64 slots:
// the former dependent chains waited out ~16 round trips, 5.7 us per call),
// then the 4 wave sums are added in order
__global__ __launch_bounds__(256) void chan_fin_kernel(const double* __restrict__ part, int slots, int C, int mode,
                                                       double* __restrict__ acc, float* __restrict__ out,
                                                       int accumulate) {
  __shared__ double red[4][64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int t = blockIdx.x * 64 + lane;
  const bool ok = t < 2 * C && !(mode == 2 && t >= C);
  double sum = 0.0;
  if (ok) {
    for (int k0 = w; k0 < slots; k0 += 64) {
      double v[16];
#pragma unroll
      for (int u = 0; u < 16; ++u) {
        const int k = k0 + 4 * u;
        v[u] = k < slots ? part[(size_t)k * 2 * C + t] : 0.0;
      }
#pragma unroll
      for (int u = 0; u < 16; ++u) sum += v[u];
    }
  }
  red[w][lane] = sum;
  __syncthreads();
  if (w == 0 && ok) {
    const double v = ((red[0][lane] + red[1][lane]) + red[2][lane]) + red[3][lane];
    if (mode == 2) out[t] = (accumulate ? out[t] : 0.f) + (float)v;
    else acc[t] = v;
  }
}

template <typename TA = float, typename TX = float>
static int chan_reduce2(const TA* a, int a_cs, int a_coff, const TX* x, int x_cs, int x_coff, const float* mean,
                        const float* invstd, const float* gamma, const float* beta, int M, int C, int mode,
                        double* part, double* acc, float* out, int accumulate, hipStream_t st) {
  const int R = kRedThreads / (C / 4);
  int slots = M / (R * 16);
  slots = slots < 1 ? 1 : (slots > kRedSlots ? kRedSlots : slots);
  hipLaunchKernelGGL((chan_part_kernel<TA, TX>), dim3(slots), dim3(kRedThreads), (size_t)R * 2 * C * sizeof(double), st, a, a_cs,
                     a_coff, x, x_cs, x_coff, mean, invstd, gamma, beta, M, C, mode, part);
  UPR_CHECK_HIP(hipGetLastError());
  hipLaunchKernelGGL(chan_fin_kernel, dim3((2 * C + 63) / 64), dim3(256), 0, st, part, slots, C, mode, acc, out,
                     accumulate);
  return (int)hipGetLastError();
}

// chan_fin (mode 0) and bn_finalize in one launch: a block owns 32 channels,
// lanes 0-31 their sums and 32-63 their sums of squares (the same slot order
// and partial-sum tree as chan_fin: bit-identical acc), then lanes 0-31
// finalise their channel as bn_finalize_kernel does
__global__ __launch_bounds__(256) void chan_fin_bn_kernel(const double* __restrict__ part, int slots, int C,
                                                          double* __restrict__ acc, int M, float momentum, float eps,
                                                          float* __restrict__ rm, float* __restrict__ rv,
                                                          long long* nbt, float* __restrict__ mean,
                                                          float* __restrict__ invstd) {
  __shared__ double red[4][64];
  __shared__ double fin[64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int c = blockIdx.x * 32 + (lane & 31);
  const bool ok = c < C;
  const int t = lane < 32 ? c : C + c;
  double sum = 0.0;  // (chan_fin_kernel's order and batching)
  if (ok) {
    for (int k0 = w; k0 < slots; k0 += 64) {
      double v[16];
#pragma unroll
      for (int u = 0; u < 16; ++u) {
        const int k = k0 + 4 * u;
        v[u] = k < slots ? part[(size_t)k * 2 * C + t] : 0.0;
      }
#pragma unroll
      for (int u = 0; u < 16; ++u) sum += v[u];
    }
  }
  red[w][lane] = sum;
  __syncthreads();
  if (w == 0) {
    const double v = ((red[0][lane] + red[1][lane]) + red[2][lane]) + red[3][lane];
    fin[lane] = v;
    if (ok) acc[t] = v;
  }
  __syncthreads();
  if (blockIdx.x == 0 && threadIdx.x == 0 && nbt) *nbt += 1;
  if (w != 0 || lane >= 32 || !ok) return;
  const double mu = fin[lane] / M;
  double var = fin[lane + 32] / M - mu * mu;
  if (var < 0) var = 0;
  mean[c] = (float)mu;
  invstd[c] = (float)(1.0 / sqrt(var + (double)eps));
  if (rm) rm[c] = (1.f - momentum) * rm[c] + momentum * (float)mu;
  if (rv) {
    const double unb = M > 1 ? var * M / (M - 1) : var;
    rv[c] = (1.f - momentum) * rv[c] + momentum * (float)unb;
  }
}

__global__ void bn_finalize_kernel(const double* __restrict__ acc, int M, int C, float momentum, float eps,
                                   float* __restrict__ rm, float* __restrict__ rv, long long* nbt,
                                   float* __restrict__ mean, float* __restrict__ invstd) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c == 0 && nbt) *nbt += 1;
  if (c >= C) return;
  const double mu = acc[c] / M;
  double var = acc[C + c] / M - mu * mu;
  if (var < 0) var = 0;
  mean[c] = (float)mu;
  invstd[c] = (float)(1.0 / sqrt(var + (double)eps));
  if (rm) rm[c] = (1.f - momentum) * rm[c] + momentum * (float)mu;
  if (rv) {
    const double unb = M > 1 ? var * M / (M - 1) : var;
    rv[c] = (1.f - momentum) * rv[c] + momentum * (float)unb;
  }
}

// eval-mode BatchNorm statistics: mean = running_mean, invstd = 1/sqrt(running_var + eps)
__global__ void bn_eval_stats_kernel(const float* __restrict__ rm, const float* __restrict__ rv, int C, float eps,
                                     float* __restrict__ mean, float* __restrict__ invstd) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  mean[c] = rm[c];
  invstd[c] = (float)(1.0 / sqrt((double)rv[c] + (double)eps));
}

__global__ __launch_bounds__(256) void bn_apply_kernel(const float* __restrict__ x, int M, int C, int x_cs,
                                                       int x_coff, const float* __restrict__ mean,
                                                       const float* __restrict__ invstd,
                                                       const float* __restrict__ gamma,
                                                       const float* __restrict__ beta, const float* res, int res_cs,
                                                       int res_coff, int res_post, int relu, float* y, int y_cs,
                                                       int y_coff) {
  const long long n = (long long)M * C;
  GSTRIDE(i, n) {
    const int c = (int)(i % C);
    const long long m = i / C;
    float v = bn_affine(x[m * x_cs + x_coff + c], mean[c], invstd[c], gamma[c], beta[c]);
    const float rv = res ? res[m * res_cs + res_coff + c] : 0.f;
    if (!res_post) v += rv;
    if (relu) v = fmaxf(v, 0.f);
    if (res_post) v += rv;
    y[m * y_cs + y_coff + c] = v;
  }
}

// the same arithmetic, 4 channels per thread (16-byte loads / stores), and
// optionally the compact fp16 copy y16[m][C] the next autocast conv reads
template <typename TX = float>
__global__ __launch_bounds__(256) void bn_apply4_kernel(const TX* __restrict__ x, int M, int C, int x_cs, int x_coff,
                                                        const float* __restrict__ mean,
                                                        const float* __restrict__ invstd,
                                                        const float* __restrict__ gamma,
                                                        const float* __restrict__ beta, const float* res, int res_cs,
                                                        int res_coff, int res_post, int relu, float* y, int y_cs,
                                                        int y_coff, half_t* __restrict__ y16, int skip32 = 0,
                                                        int y16_cs = 0) {
  const int C4 = C / 4;
  const int ycs16 = y16_cs > 0 ? y16_cs : C;  // y16: compact [M][C], or a channel slice of a wider copy
  if (256 % C4 == 0) {
    // this thread's 4 channels are fixed (the grid stride is a multiple of C4):
    // per-channel parameters once, row index by addition -- no div / mod per
    // element (the 64-bit form ran at ~3 TB/s); 32-bit offsets (host-checked)
    const int c = (threadIdx.x % C4) * 4, rpb = 256 / C4;
    float mu[4], is[4], ga[4], be[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) { mu[e] = mean[c + e]; is[e] = invstd[c + e]; ga[e] = gamma[c + e]; be[e] = beta[c + e]; }
    for (int m = blockIdx.x * rpb + threadIdx.x / C4; m < M; m += gridDim.x * rpb) {
      const float4 xv = ld4f(x + (size_t)m * x_cs + x_coff + c);
      const float4 rv4 = res ? *(const float4*)(res + (size_t)m * res_cs + res_coff + c) : make_float4(0.f, 0.f, 0.f, 0.f);
      const float xa[4] = {xv.x, xv.y, xv.z, xv.w}, ra[4] = {rv4.x, rv4.y, rv4.z, rv4.w};
      float o[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float v = bn_affine(xa[e], mu[e], is[e], ga[e], be[e]);
        if (!res_post) v += ra[e];
        if (relu) v = fmaxf(v, 0.f);
        if (res_post) v += ra[e];
        o[e] = v;
      }
      if (!skip32) *(float4*)(y + (size_t)m * y_cs + y_coff + c) = make_float4(o[0], o[1], o[2], o[3]);
      if (y16) {
        typedef _Float16 h4 __attribute__((ext_vector_type(4)));
        *(h4*)(y16 + (size_t)m * ycs16 + c) = h4{(half_t)o[0], (half_t)o[1], (half_t)o[2], (half_t)o[3]};
      }
    }
    return;
  }
  const long long n = (long long)M * C4;
  GSTRIDE(i, n) {
    const int c = (int)(i % C4) * 4;
    const long long m = i / C4;
    const float4 xv = ld4f(x + m * x_cs + x_coff + c);
    const float4 rv4 = res ? *(const float4*)(res + m * res_cs + res_coff + c) : make_float4(0.f, 0.f, 0.f, 0.f);
    const float xa[4] = {xv.x, xv.y, xv.z, xv.w}, ra[4] = {rv4.x, rv4.y, rv4.z, rv4.w};
    float o[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float v = bn_affine(xa[e], mean[c + e], invstd[c + e], gamma[c + e], beta[c + e]);
      if (!res_post) v += ra[e];
      if (relu) v = fmaxf(v, 0.f);
      if (res_post) v += ra[e];
      o[e] = v;
    }
    if (!skip32) *(float4*)(y + m * y_cs + y_coff + c) = make_float4(o[0], o[1], o[2], o[3]);
    if (y16) {
      typedef _Float16 h4 __attribute__((ext_vector_type(4)));
      *(h4*)(y16 + m * ycs16 + c) = h4{(half_t)o[0], (half_t)o[1], (half_t)o[2], (half_t)o[3]};
    }
  }
}

__global__ __launch_bounds__(256) void bn_bwd_apply_kernel(const float* __restrict__ g, int g_cs, int g_coff,
                                                           const float* __restrict__ x, int x_cs, int x_coff,
                                                           const float* __restrict__ mean,
                                                           const float* __restrict__ invstd,
                                                           const float* __restrict__ gamma,
                                                           const double* __restrict__ acc, int M, int C,
                                                           float* dgamma, float* dbeta, float* dx, int dx_cs,
                                                           int dx_coff, int accum, int batch_stats) {
  if (blockIdx.x == 0) {
    for (int c = threadIdx.x; c < C; c += blockDim.x) {
      if (dgamma) dgamma[c] += (float)acc[C + c];
      if (dbeta) dbeta[c] += (float)acc[c];
    }
  }
  const long long n = (long long)M * C;
  GSTRIDE(i, n) {
    const int c = (int)(i % C);
    const long long m = i / C;
    const float is = invstd[c];
    const float xh = (x[m * x_cs + x_coff + c] - mean[c]) * is;
    // batch statistics: the mean / x-hat terms of the batch-statistics backward;
    // running statistics (an eval-mode BN): the plain affine map g * gamma * invstd
    const float sg = batch_stats ? (float)(acc[c] / M) : 0.f, sgx = batch_stats ? (float)(acc[C + c] / M) : 0.f;
    float v = gamma[c] * is * (g[m * g_cs + g_coff + c] - sg - xh * sgx);
    float* o = dx + m * dx_cs + dx_coff + c;
    if (accum) v += *o;
    *o = v;
  }
}

// the same arithmetic, 4 channels per thread (16-byte loads / stores)
template <typename TX = float, typename TG = float>
__global__ __launch_bounds__(256) void bn_bwd_apply4_kernel(const TG* __restrict__ g, int g_cs, int g_coff,
                                                            const TX* __restrict__ x, int x_cs, int x_coff,
                                                            const float* __restrict__ mean,
                                                            const float* __restrict__ invstd,
                                                            const float* __restrict__ gamma,
                                                            const double* __restrict__ acc, int M, int C,
                                                            float* dgamma, float* dbeta, float* dx, int dx_cs,
                                                            int dx_coff, int accum, int batch_stats,
                                                            const float* __restrict__ beta = nullptr, int relu = 0,
                                                            half_t* __restrict__ dx16 = nullptr, int skip32 = 0) {
  // relu: the consumer ReLU folded in (g counts where bn(x) > 0, recomputed);
  // dx16: compact [M][C] fp16 copy of dx for the autocast input-gradient conv
  if (blockIdx.x == 0) {
    for (int c = threadIdx.x; c < C; c += blockDim.x) {
      if (dgamma) dgamma[c] += (float)acc[C + c];
      if (dbeta) dbeta[c] += (float)acc[c];
    }
  }
  const int C4 = C / 4;
  if (256 % C4 == 0) {
    // fixed channels per thread (see bn_apply4_kernel): the per-channel terms,
    // fp64 divides included, once per thread instead of per element
    const int c = (threadIdx.x % C4) * 4, rpb = 256 / C4;
    // every per-channel load unconditional and issued together, the flags applied
    // by selects, 1/M one uniform divide: the conditional-load form (a branch and
    // a full memory wait per term, fp64 divides between) ran at ~2 TB/s on the
    // training shapes, its per-thread prologue dominating a one-row thread
    const float* bp = relu ? beta : gamma;  // beta may be NULL without the fold
    const double invM = batch_stats ? 1.0 / M : 0.0;
    float mu[4], is[4], ga[4], be[4], sg[4], sgx[4], gis[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      mu[e] = mean[c + e];
      is[e] = invstd[c + e];
      ga[e] = gamma[c + e];
      const float bv = bp[c + e];
      be[e] = relu ? bv : 0.f;
      sg[e] = (float)(acc[c + e] * invM);
      sgx[e] = (float)(acc[C + c + e] * invM);
      gis[e] = ga[e] * is[e];
    }
    for (int m = blockIdx.x * rpb + threadIdx.x / C4; m < M; m += gridDim.x * rpb) {
      const float4 gv = ld4f(g + (size_t)m * g_cs + g_coff + c);
      const float4 xv = ld4f(x + (size_t)m * x_cs + x_coff + c);
      const float ga4[4] = {gv.x, gv.y, gv.z, gv.w}, xa[4] = {xv.x, xv.y, xv.z, xv.w};
      float4* o = (float4*)(dx + (size_t)m * dx_cs + dx_coff + c);
      const float4 prev = accum ? *o : make_float4(0.f, 0.f, 0.f, 0.f);
      const float pa[4] = {prev.x, prev.y, prev.z, prev.w};
      float r[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float xh = (xa[e] - mu[e]) * is[e];
        float gg = ga4[e];
        if (relu && !(bn_affine(xa[e], mu[e], is[e], ga[e], be[e]) > 0.f)) gg = 0.f;
        float v = gis[e] * (gg - sg[e] - xh * sgx[e]);
        if (accum) v += pa[e];
        r[e] = v;
      }
      if (!skip32) *o = make_float4(r[0], r[1], r[2], r[3]);
      if (dx16) {
        typedef _Float16 h4 __attribute__((ext_vector_type(4)));
        *(h4*)(dx16 + (size_t)m * C + c) = h4{(half_t)r[0], (half_t)r[1], (half_t)r[2], (half_t)r[3]};
      }
    }
    return;
  }
  const long long n = (long long)M * C4;
  GSTRIDE(i, n) {
    const int c = (int)(i % C4) * 4;
    const long long m = i / C4;
    const float4 gv = ld4f(g + m * g_cs + g_coff + c);
    const float4 xv = ld4f(x + m * x_cs + x_coff + c);
    const float ga[4] = {gv.x, gv.y, gv.z, gv.w}, xa[4] = {xv.x, xv.y, xv.z, xv.w};
    float4* o = (float4*)(dx + m * dx_cs + dx_coff + c);
    float4 prev = accum ? *o : make_float4(0.f, 0.f, 0.f, 0.f);
    const float pa[4] = {prev.x, prev.y, prev.z, prev.w};
    float r[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float is = invstd[c + e];
      const float xh = (xa[e] - mean[c + e]) * is;
      const float sg = batch_stats ? (float)(acc[c + e] / M) : 0.f;
      const float sgx = batch_stats ? (float)(acc[C + c + e] / M) : 0.f;
      float gg = ga[e];
      if (relu && !(bn_affine(xa[e], mean[c + e], is, gamma[c + e], beta[c + e]) > 0.f)) gg = 0.f;
      float v = gamma[c + e] * is * (gg - sg - xh * sgx);
      if (accum) v += pa[e];
      r[e] = v;
    }
    if (!skip32) *o = make_float4(r[0], r[1], r[2], r[3]);
    if (dx16) {
      typedef _Float16 h4 __attribute__((ext_vector_type(4)));
      *(h4*)(dx16 + m * C + c) = h4{(half_t)r[0], (half_t)r[1], (half_t)r[2], (half_t)r[3]};
    }
  }
}

}  // namespace upr

using namespace upr;

extern "C" {

int upr_t_bn_stats(const float* x, int M, int C, int cs, int coff, double* acc, void* stream) {
  if (!x || !acc || M <= 0 || C <= 0) return UPR_ERR_ARG;
  if (reduce4_ok(C, cs, coff, x))
    return chan_reduce2(x, cs, coff, (const float*)nullptr, 0, 0, nullptr, nullptr, nullptr, nullptr, M, C, 0,
                        acc + 2 * C, acc, nullptr, 0, ST(stream));
  // the atomic fallback adds into acc: cleared here, so every path overwrites
  UPR_CHECK_HIP(hipMemsetAsync(acc, 0, sizeof(double) * 2 * C, ST(stream)));
  hipLaunchKernelGGL(chan_reduce_kernel, dim3(reduce_grid(M)), dim3(256), 0, ST(stream), x, cs, coff, nullptr, 0, 0,
                     nullptr, nullptr, M, C, 0, acc, nullptr);
  LAUNCH_CHECK();
}

int upr_t_bn_finalize(const double* acc, int M, int C, float momentum, float eps, float* running_mean,
                      float* running_var, int64_t* nbt, float* mean, float* invstd, void* stream) {
  if (!acc || !mean || !invstd || M <= 0) return UPR_ERR_ARG;
  hipLaunchKernelGGL(bn_finalize_kernel, dim3((C + 255) / 256), dim3(256), 0, ST(stream), acc, M, C, momentum, eps,
                     running_mean, running_var, (long long*)nbt, mean, invstd);
  LAUNCH_CHECK();
}

int upr_t_bn_eval_stats(const float* running_mean, const float* running_var, int C, float eps, float* mean,
                        float* invstd, void* stream) {
  if (!running_mean || !running_var || !mean || !invstd || C <= 0) return UPR_ERR_ARG;
  hipLaunchKernelGGL(bn_eval_stats_kernel, dim3((C + 255) / 256), dim3(256), 0, ST(stream), running_mean, running_var, C,
                     eps, mean, invstd);
  LAUNCH_CHECK();
}

int upr_t_bn_apply16(const float* x, int M, int C, int x_cs, int x_coff, const float* mean, const float* invstd,
                     const float* gamma, const float* beta, const float* res, int res_cs, int res_coff, int res_post,
                     int relu, float* y, int y_cs, int y_coff, void* y16, void* stream) {
  if (!x || !y || !mean || !invstd || !gamma || !beta) return UPR_ERR_ARG;
  const auto a16 = [](const void* p) { return ((uintptr_t)p & 15) == 0; };
  const bool v4 = C % 4 == 0 && x_cs % 4 == 0 && x_coff % 4 == 0 && y_cs % 4 == 0 && y_coff % 4 == 0 && a16(x) &&
                  a16(y) && (!res || (res_cs % 4 == 0 && res_coff % 4 == 0 && a16(res))) &&
                  (!y16 || ((uintptr_t)y16 & 7) == 0);
  if (v4) {
    const long long n4 = (long long)M * (C / 4);
    hipLaunchKernelGGL(bn_apply4_kernel<float>, dim3(grid_for(n4)), dim3(256), 0, ST(stream), x, M, C, x_cs, x_coff, mean,
                       invstd, gamma, beta, res, res_cs, res_coff, res_post, relu, y, y_cs, y_coff, (half_t*)y16);
    LAUNCH_CHECK();
  }
  if (y16) return UPR_ERR_ARG;  // the fp16 copy needs the vectorised layout
  const long long n = (long long)M * C;
  hipLaunchKernelGGL(bn_apply_kernel, dim3(grid_for(n)), dim3(256), 0, ST(stream), x, M, C, x_cs, x_coff, mean,
                     invstd, gamma, beta, res, res_cs, res_coff, res_post, relu, y, y_cs, y_coff);
  LAUNCH_CHECK();
}

int upr_t_bn_apply(const float* x, int M, int C, int x_cs, int x_coff, const float* mean, const float* invstd,
                   const float* gamma, const float* beta, const float* res, int res_cs, int res_coff, int res_post,
                   int relu, float* y, int y_cs, int y_coff, void* stream) {
  return upr_t_bn_apply16(x, M, C, x_cs, x_coff, mean, invstd, gamma, beta, res, res_cs, res_coff, res_post, relu, y,
                          y_cs, y_coff, nullptr, stream);
}

int upr_t_bn_bwd_reduce(const float* g, int g_cs, int g_coff, const float* x, int x_cs, int x_coff, const float* mean,
                        const float* invstd, int M, int C, double* acc, void* stream) {
  if (!g || !x || !acc) return UPR_ERR_ARG;
  if (reduce4_ok(C, g_cs, g_coff, g) && reduce4_ok(C, x_cs, x_coff, x))
    return chan_reduce2(g, g_cs, g_coff, x, x_cs, x_coff, mean, invstd, nullptr, nullptr, M, C, 1, acc + 2 * C, acc,
                        nullptr, 0, ST(stream));
  else
    hipLaunchKernelGGL(chan_reduce_kernel, dim3(reduce_grid(M)), dim3(256), 0, ST(stream), g, g_cs, g_coff, x, x_cs,
                       x_coff, mean, invstd, M, C, 1, acc, nullptr);
  LAUNCH_CHECK();
}

int upr_t_bn_bwd_apply(const float* g, int g_cs, int g_coff, const float* x, int x_cs, int x_coff, const float* mean,
                       const float* invstd, const float* gamma, const double* acc, int M, int C, float* dgamma,
                       float* dbeta, float* dx, int dx_cs, int dx_coff, int accumulate, int batch_stats,
                       void* stream) {
  if (!g || !x || !acc || !dx || !gamma) return UPR_ERR_ARG;
  const auto a16 = [](const void* p) { return ((uintptr_t)p & 15) == 0; };
  if (C % 4 == 0 && g_cs % 4 == 0 && g_coff % 4 == 0 && x_cs % 4 == 0 && x_coff % 4 == 0 && dx_cs % 4 == 0 &&
      dx_coff % 4 == 0 && a16(g) && a16(x) && a16(dx)) {
    const long long n4 = (long long)M * (C / 4);
    hipLaunchKernelGGL((bn_bwd_apply4_kernel<float, float>), dim3(grid_for(n4)), dim3(256), 0, ST(stream), g, g_cs, g_coff, x, x_cs,
                       x_coff, mean, invstd, gamma, acc, M, C, dgamma, dbeta, dx, dx_cs, dx_coff, accumulate,
                       batch_stats);
    LAUNCH_CHECK();
  }
  const long long n = (long long)M * C;
  hipLaunchKernelGGL(bn_bwd_apply_kernel, dim3(grid_for(n)), dim3(256), 0, ST(stream), g, g_cs, g_coff, x, x_cs,
                     x_coff, mean, invstd, gamma, acc, M, C, dgamma, dbeta, dx, dx_cs, dx_coff, accumulate,
                       batch_stats);
  LAUNCH_CHECK();
}

int upr_t_bn_bwd_fused(const float* g, int g_cs, int g_coff, const float* x, int x_cs, const float* mean,
                       const float* invstd, const float* gamma, const float* beta, int relu, int M, int C,
                       double* acc, float* dgamma, float* dbeta, float* dx, int dx_cs, int dx_coff, int accumulate,
                       int batch_stats, void* dx16, void* stream) {
  if (!g || !x || !acc || !dx || !gamma || !beta || !mean || !invstd || M <= 0 || C <= 0) return UPR_ERR_ARG;
  const auto a16 = [](const void* p) { return ((uintptr_t)p & 15) == 0; };
  if (C % 4 || C > 1024 || g_cs % 4 || g_coff % 4 || x_cs % 4 || dx_cs % 4 || dx_coff % 4 || !a16(g) || !a16(x) ||
      !a16(dx) || !a16(mean) || !a16(invstd) || !a16(gamma) || !a16(beta) || ((uintptr_t)dx16 & 7))
    return UPR_ERR_UNSUPPORTED;
  hipStream_t st = ST(stream);
  const int rc = chan_reduce2(g, g_cs, g_coff, x, x_cs, 0, mean, invstd, gamma, beta, M, C, relu ? 3 : 1, acc + 2 * C,
                              acc, nullptr, 0, st);
  if (rc) return rc;
  const long long n4 = (long long)M * (C / 4);
  hipLaunchKernelGGL((bn_bwd_apply4_kernel<float, float>), dim3(grid_for(n4)), dim3(256), 0, st, g, g_cs, g_coff, x, x_cs, 0, mean,
                     invstd, gamma, acc, M, C, dgamma, dbeta, dx, dx_cs, dx_coff, accumulate, batch_stats, beta, relu,
                     (half_t*)dx16);
  LAUNCH_CHECK();
}

// x read from its compact fp16 copy x16 ([M][C]; under autocast the BN input
// is an fp16 conv's output, whose fp32 form holds the same values)
int upr_t_bn_stats16(const void* x16, int M, int C, double* acc, void* stream) {
  if (!x16 || !acc || M <= 0 || C <= 0) return UPR_ERR_ARG;
  if (C % 4 || C > 1024 || (uintptr_t)x16 % 8) return UPR_ERR_UNSUPPORTED;
  return chan_reduce2((const half_t*)x16, C, 0, (const float*)nullptr, 0, 0, nullptr, nullptr, nullptr, nullptr, M, C,
                      0, acc + 2 * C, acc, nullptr, 0, ST(stream));
}

int upr_t_bn_stats16_fin(const void* x16, int M, int C, double* acc, float momentum, float eps, float* running_mean,
                         float* running_var, int64_t* nbt, float* mean, float* invstd, void* stream) {
  if (!x16 || !acc || !mean || !invstd || M <= 0 || C <= 0) return UPR_ERR_ARG;
  if (C % 4 || C > 1024 || (uintptr_t)x16 % 8) return UPR_ERR_UNSUPPORTED;
  hipStream_t st = ST(stream);
  const int R = kRedThreads / (C / 4);
  int slots = M / (R * 16);
  slots = slots < 1 ? 1 : (slots > kRedSlots ? kRedSlots : slots);
  double* part = acc + 2 * C;
  hipLaunchKernelGGL((chan_part_kernel<half_t, float>), dim3(slots), dim3(kRedThreads),
                     (size_t)R * 2 * C * sizeof(double), st, (const half_t*)x16, C, 0, (const float*)nullptr, 0, 0,
                     nullptr, nullptr, nullptr, nullptr, M, C, 0, part);
  UPR_CHECK_HIP(hipGetLastError());
  hipLaunchKernelGGL(chan_fin_bn_kernel, dim3((C + 31) / 32), dim3(256), 0, st, (const double*)part, slots, C, acc, M,
                     momentum, eps, running_mean, running_var, (long long*)nbt, mean, invstd);
  LAUNCH_CHECK();
}

int upr_t_bn_apply16h_cs(const void* x16, int M, int C, const float* mean, const float* invstd, const float* gamma,
                         const float* beta, const float* res, int res_cs, int res_coff, int res_post, int relu,
                         float* y, int y_cs, int y_coff, void* y16, int y16_cs, int skip32, void* stream) {
  if (!x16 || !y || !mean || !invstd || !gamma || !beta || M <= 0 || C <= 0) return UPR_ERR_ARG;
  if (skip32 && !y16) return UPR_ERR_ARG;
  if (y16_cs < 0 || (y16_cs > 0 && y16_cs < C)) return UPR_ERR_ARG;
  const auto a16 = [](const void* p) { return ((uintptr_t)p & 15) == 0; };
  if (C % 4 || (uintptr_t)x16 % 8 || y_cs % 4 || y_coff % 4 || !a16(y) ||
      (res && (res_cs % 4 || res_coff % 4 || !a16(res))) || ((uintptr_t)y16 & 7) || y16_cs % 4)
    return UPR_ERR_UNSUPPORTED;
  const long long n4 = (long long)M * (C / 4);
  hipLaunchKernelGGL(bn_apply4_kernel<half_t>, dim3(grid_for(n4)), dim3(256), 0, ST(stream), (const half_t*)x16, M, C,
                     C, 0, mean, invstd, gamma, beta, res, res_cs, res_coff, res_post, relu, y, y_cs, y_coff,
                     (half_t*)y16, skip32, y16_cs);
  LAUNCH_CHECK();
}

int upr_t_bn_apply16h(const void* x16, int M, int C, const float* mean, const float* invstd, const float* gamma,
                      const float* beta, const float* res, int res_cs, int res_coff, int res_post, int relu, float* y,
                      int y_cs, int y_coff, void* y16, int skip32, void* stream) {
  return upr_t_bn_apply16h_cs(x16, M, C, mean, invstd, gamma, beta, res, res_cs, res_coff, res_post, relu, y, y_cs,
                              y_coff, y16, 0, skip32, stream);
}

int upr_t_bn_bwd_fused16(const float* g, const void* g16, int g_cs, int g_coff, const void* x16, const float* mean,
                         const float* invstd, const float* gamma, const float* beta, int relu, int M, int C,
                         double* acc, float* dgamma, float* dbeta, float* dx, int dx_cs, int dx_coff, int accumulate,
                         int batch_stats, void* dx16, int skip32, void* stream) {
  if ((!g && !g16) || !x16 || !acc || !dx || !gamma || !beta || !mean || !invstd || M <= 0 || C <= 0)
    return UPR_ERR_ARG;
  if (skip32 && (accumulate || !dx16)) return UPR_ERR_ARG;
  const auto a16 = [](const void* p) { return ((uintptr_t)p & 15) == 0; };
  if (C % 4 || C > 1024 || dx_cs % 4 || dx_coff % 4 || (uintptr_t)x16 % 8 || !a16(dx) || !a16(mean) ||
      !a16(invstd) || !a16(gamma) || !a16(beta) || ((uintptr_t)dx16 & 7))
    return UPR_ERR_UNSUPPORTED;
  if (g16 ? (uintptr_t)g16 % 8 != 0 : (g_cs % 4 || g_coff % 4 || !a16(g))) return UPR_ERR_UNSUPPORTED;
  hipStream_t st = ST(stream);
  const long long n4 = (long long)M * (C / 4);
  if (g16) {  // g = the input-gradient conv's fp16 output (compact [M][C])
    const int rc = chan_reduce2((const half_t*)g16, C, 0, (const half_t*)x16, C, 0, mean, invstd, gamma, beta, M, C,
                                relu ? 3 : 1, acc + 2 * C, acc, nullptr, 0, st);
    if (rc) return rc;
    hipLaunchKernelGGL((bn_bwd_apply4_kernel<half_t, half_t>), dim3(grid_for(n4)), dim3(256), 0, st,
                       (const half_t*)g16, C, 0, (const half_t*)x16, C, 0, mean, invstd, gamma, acc, M, C, dgamma,
                       dbeta, dx, dx_cs, dx_coff, accumulate, batch_stats, beta, relu, (half_t*)dx16, skip32);
    LAUNCH_CHECK();
  }
  const int rc = chan_reduce2(g, g_cs, g_coff, (const half_t*)x16, C, 0, mean, invstd, gamma, beta, M, C,
                              relu ? 3 : 1, acc + 2 * C, acc, nullptr, 0, st);
  if (rc) return rc;
  hipLaunchKernelGGL((bn_bwd_apply4_kernel<half_t, float>), dim3(grid_for(n4)), dim3(256), 0, st, g, g_cs, g_coff,
                     (const half_t*)x16, C, 0, mean, invstd, gamma, acc, M, C, dgamma, dbeta, dx, dx_cs, dx_coff,
                     accumulate, batch_stats, beta, relu, (half_t*)dx16, skip32);
  LAUNCH_CHECK();
}

int upr_t_chan_sum(const float* g, int M, int C, int cs, int coff, float* out, int accumulate, void* stream) {
  if (!g || !out) return UPR_ERR_ARG;
  if (!accumulate) UPR_CHECK_HIP(hipMemsetAsync(out, 0, sizeof(float) * C, ST(stream)));
  if (reduce4_ok(C, cs, coff, g)) {
    hipLaunchKernelGGL(chan_reduce4_kernel, dim3(reduce_grid(M)), dim3(256), 0, ST(stream), g, cs, coff, nullptr, 0, 0,
                       nullptr, nullptr, M, C, 2, nullptr, out);
    LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(chan_reduce_kernel, dim3(reduce_grid(M)), dim3(256), 0, ST(stream), g, cs, coff, nullptr, 0, 0,
                     nullptr, nullptr, M, C, 2, nullptr, out);
  LAUNCH_CHECK();
}

int upr_t_chan_sum_ws(const float* g, int M, int C, int cs, int coff, float* out, int accumulate, double* ws,
                      void* stream) {
  if (!g || !out || !ws || M <= 0 || C <= 0) return UPR_ERR_ARG;
  if (!reduce4_ok(C, cs, coff, g)) return upr_t_chan_sum(g, M, C, cs, coff, out, accumulate, stream);
  return chan_reduce2(g, cs, coff, (const float*)nullptr, 0, 0, nullptr, nullptr, nullptr, nullptr, M, C, 2, ws, nullptr, out,
                      accumulate, ST(stream));
}

int upr_t_chan_sum16(const void* g16, int M, int C, float* out, int accumulate, double* ws, void* stream) {
  if (!g16 || !out || !ws || M <= 0 || C <= 0) return UPR_ERR_ARG;
  if (C % 4 || C > 1024 || (uintptr_t)g16 % 8) return UPR_ERR_UNSUPPORTED;
  return chan_reduce2((const half_t*)g16, C, 0, (const float*)nullptr, 0, 0, nullptr, nullptr, nullptr, nullptr, M, C,
                      2, ws, nullptr, out, accumulate, ST(stream));
}

int upr_t_chan_sum16s(const void* g16, int M, int C, int cs, float* out, int accumulate, double* ws, void* stream) {
  if (!g16 || !out || !ws || M <= 0 || C <= 0 || cs < C) return UPR_ERR_ARG;
  if (C % 4 || C > 1024 || cs % 4 || (uintptr_t)g16 % 8) return UPR_ERR_UNSUPPORTED;
  return chan_reduce2((const half_t*)g16, cs, 0, (const float*)nullptr, 0, 0, nullptr, nullptr, nullptr, nullptr, M, C,
                      2, ws, nullptr, out, accumulate, ST(stream));
}

int upr_t_reduce_acc_doubles(int C) { return 2 * C * (1 + kRedSlots); }

}  // extern "C"
