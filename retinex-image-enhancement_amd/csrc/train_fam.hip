// EnhancedFAM attention for gfx950 (one thread per pixel, C channels
// contiguous; C == 32 forms: 8 lanes per pixel) and the network tail (head,
// retinex, enhance).
// Entries: include/upr_train.h; layout and precision: train_common.h.
#include <cmath>

#include "train_common.h"

namespace upr {

// ---------------------------------------------------------------------------
// EnhancedFAM attention (one thread per pixel, C channels contiguous)
// ---------------------------------------------------------------------------
__global__ void fam_ca_apply_kernel(const float* __restrict__ o, const float* __restrict__ ca, int B, int HW, int C,
                                    float* __restrict__ o2, float* __restrict__ m) {
  const long long n = (long long)B * HW;
  GSTRIDE(i, n) {
    const int b = (int)(i / HW);
    const float* op = o + i * C;
    float* q = o2 + i * C;
    float s = 0.f, mx = -INFINITY;
    for (int c = 0; c < C; ++c) {
      const float v = op[c] * ca[(size_t)b * C + c];
      q[c] = v;
      s += v;
      if (v > mx || isnan(v)) mx = v;
    }
    m[i * 2] = s / (float)C;
    m[i * 2 + 1] = mx;
  }
}

__global__ void fam_sa_apply_kernel(const float* __restrict__ o2, const float* __restrict__ s_pre, int B, int HW, int C,
                                    float* __restrict__ sa, float* __restrict__ out) {
  const long long n = (long long)B * HW;
  GSTRIDE(i, n) {
    const float a = 1.f / (1.f + expf(-s_pre[i]));
    sa[i] = a;
    for (int c = 0; c < C; ++c) out[i * C + c] = o2[i * C + c] * a;
  }
}

__global__ void fam_sa_bwd_kernel(const float* __restrict__ g, int g_cs, const float* __restrict__ o2,
                                  const float* __restrict__ sa, int B, int HW, int C, float* __restrict__ g_o2,
                                  float* __restrict__ g_spre) {
  const long long n = (long long)B * HW;
  GSTRIDE(i, n) {
    const float a = sa[i];
    float t = 0.f;
    for (int c = 0; c < C; ++c) {
      const float gv = g[i * g_cs + c];
      t += gv * o2[i * C + c];
      g_o2[i * C + c] = gv * a;
    }
    g_spre[i] = t * a * (1.f - a);
  }
}

// C == 32 forms of the three per-pixel attention kernels above: 8 lanes per
// pixel, one float4 per lane (a wave reads 8 whole 128-byte pixel rows per
// instruction instead of 64 lanes striding 128 B apart), the channel mean / max /
// dot reduced over the 8-lane group by xor shuffles.  Groups of 8 are aligned
// (n and blockDim multiples of 8), so a whole group leaves the loop together.
__device__ __forceinline__ float nanmax(float a, float b) { return (b > a || isnan(b)) ? b : a; }

__global__ void fam_ca_apply32_kernel(const float* __restrict__ o, const float* __restrict__ ca, int B, int HW,
                                      float* __restrict__ o2, float* __restrict__ m) {
  const long long n = (long long)B * HW * 8;
  GSTRIDE(i, n) {
    const long long pix = i >> 3;
    const int q = (int)(i & 7);
    const int b = (int)(pix / HW);
    float4 v = ((const float4*)(o + pix * 32))[q];
    const float4 w = ((const float4*)(ca + (size_t)b * 32))[q];
    v.x *= w.x; v.y *= w.y; v.z *= w.z; v.w *= w.w;
    ((float4*)(o2 + pix * 32))[q] = v;
    float sm = (v.x + v.y) + (v.z + v.w);
    float mx = nanmax(nanmax(v.x, v.y), nanmax(v.z, v.w));
    for (int off = 1; off < 8; off <<= 1) {
      sm += __shfl_xor(sm, off);
      mx = nanmax(mx, __shfl_xor(mx, off));
    }
    if (q == 0) {
      m[pix * 2] = sm / 32.f;
      m[pix * 2 + 1] = mx;
    }
  }
}

__global__ void fam_sa_apply32_kernel(const float* __restrict__ o2, const float* __restrict__ s_pre, int B, int HW,
                                      float* __restrict__ sa, float* __restrict__ out) {
  const long long n = (long long)B * HW * 8;
  GSTRIDE(i, n) {
    const long long pix = i >> 3;
    const int q = (int)(i & 7);
    const float a = 1.f / (1.f + expf(-s_pre[pix]));
    if (q == 0) sa[pix] = a;
    float4 v = ((const float4*)(o2 + pix * 32))[q];
    v.x *= a; v.y *= a; v.z *= a; v.w *= a;
    ((float4*)(out + pix * 32))[q] = v;
  }
}

__global__ void fam_sa_bwd32_kernel(const float* __restrict__ g, int g_cs, const float* __restrict__ o2,
                                    const float* __restrict__ sa, int B, int HW, float* __restrict__ g_o2,
                                    float* __restrict__ g_spre) {
  const long long n = (long long)B * HW * 8;
  GSTRIDE(i, n) {
    const long long pix = i >> 3;
    const int q = (int)(i & 7);
    const float a = sa[pix];
    const float4 gv = ((const float4*)(g + pix * g_cs))[q];
    const float4 ov = ((const float4*)(o2 + pix * 32))[q];
    float t = (gv.x * ov.x + gv.y * ov.y) + (gv.z * ov.z + gv.w * ov.w);
    ((float4*)(g_o2 + pix * 32))[q] = make_float4(gv.x * a, gv.y * a, gv.z * a, gv.w * a);
    for (int off = 1; off < 8; off <<= 1) t += __shfl_xor(t, off);
    if (q == 0) g_spre[pix] = t * a * (1.f - a);
  }
}

// g_ca[b][c] partials go through LDS: a block covers a pixel range of one image
__global__ __launch_bounds__(256) void fam_ca_bwd_kernel(const float* __restrict__ g_o2, const float* __restrict__ g_m,
                                                         const float* __restrict__ o, const float* __restrict__ o2,
                                                         const float* __restrict__ ca, int HW, int C,
                                                         float* __restrict__ g_o, float* __restrict__ g_ca) {
  __shared__ float sm[256][33];
  const int b = blockIdx.y;
  const int per = (HW + gridDim.x - 1) / gridDim.x;
  const int p0 = blockIdx.x * per, p1 = min(HW, p0 + per);
  float part[32];
#pragma unroll
  for (int c = 0; c < 32; ++c) part[c] = 0.f;
  for (int q = p0 + threadIdx.x; q < p1; q += 256) {
    const size_t i = (size_t)b * HW + q;
    const float gm0 = g_m[i * 2] / (float)C, gm1 = g_m[i * 2 + 1];
    // argmax over channels of o2 (first maximum, torch.max semantics)
    int am = 0;
    float mx = o2[i * C];
    for (int c = 1; c < C; ++c) {
      const float v = o2[i * C + c];
      if (v > mx || (isnan(v) && !isnan(mx))) { mx = v; am = c; }
    }
#pragma unroll
    for (int c = 0; c < 32; ++c) {
      if (c >= C) break;
      const float gt = g_o2[i * C + c] + gm0 + (c == am ? gm1 : 0.f);
      g_o[i * C + c] = gt * ca[(size_t)b * C + c];
      part[c] += gt * o[i * C + c];
    }
  }
#pragma unroll
  for (int c = 0; c < 32; ++c) sm[threadIdx.x][c] = part[c];
  __syncthreads();
  // 8 groups of 32 threads' partials a channel, then the 8 group sums: chains
  // of 32 + 8 additions (one chain of 256 was 6.9 ulp off float64 at HW = 515)
  const int cc = threadIdx.x & 31, grp = threadIdx.x >> 5;
  float gs = 0.f;
  for (int k = 0; k < 32; ++k) gs += sm[grp * 32 + k][cc];
  __syncthreads();
  sm[grp][cc] = gs;
  __syncthreads();
  if (threadIdx.x < C) {
    float t = 0.f;
    for (int k = 0; k < 8; ++k) t += sm[k][threadIdx.x];
    atomicAdd(g_ca + (size_t)b * C + threadIdx.x, t);
  }
}

// C = 32 form: 8 lanes per pixel (a float4 of channels each, coalesced rows),
// the channel argmax reduced across the 8 lanes with the scan's rule (first
// NaN, else first maximum), per-block partial sums of gt * o in a fixed order
// to part[b][chunk][c] (summed in chunk order by fam_ca_fin_kernel: no atomics)
__device__ __forceinline__ void argmax_pick(float& v, int& i, float v2, int i2) {
  const bool second_is_later = i2 > i;
  const float fv = second_is_later ? v : v2, sv = second_is_later ? v2 : v;
  const int fi = second_is_later ? i : i2, si = second_is_later ? i2 : i;
  const bool take_second = sv > fv || (isnan(sv) && !isnan(fv));
  v = take_second ? sv : fv;
  i = take_second ? si : fi;
}

__global__ __launch_bounds__(256) void fam_ca_bwd32_kernel(const float* __restrict__ g_o2,
                                                           const float* __restrict__ g_m, const float* __restrict__ o,
                                                           const float* __restrict__ o2, const float* __restrict__ ca,
                                                           int HW, float* __restrict__ g_o, float* __restrict__ part) {
  __shared__ float sm[32][33];
  const int b = blockIdx.y, q = threadIdx.x & 7, pl = threadIdx.x >> 3;
  const int per = (HW + gridDim.x - 1) / gridDim.x;
  const int p0 = blockIdx.x * per, p1 = min(HW, p0 + per);
  const float4 cav = *(const float4*)(ca + (size_t)b * 32 + q * 4);
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  // (each pixel's four operand loads are issued together, before its argmax
  // shuffles: 99.9 -> 93.7 us per call on the training step)
  for (int p = p0 + pl; p < p1; p += 32) {
    const size_t i = (size_t)b * HW + p;
    const float4 v = *(const float4*)(o2 + i * 32 + q * 4);
    const float4 gv = *(const float4*)(g_o2 + i * 32 + q * 4);
    const float4 ov = *(const float4*)(o + i * 32 + q * 4);
    const float gm0 = g_m[i * 2] / 32.f, gm1 = g_m[i * 2 + 1];
    float mv = v.x;
    int mi = q * 4;
    argmax_pick(mv, mi, v.y, q * 4 + 1);
    argmax_pick(mv, mi, v.z, q * 4 + 2);
    argmax_pick(mv, mi, v.w, q * 4 + 3);
#pragma unroll
    for (int off = 1; off < 8; off <<= 1) {
      const float v2 = __shfl_xor(mv, off);
      const int i2 = __shfl_xor(mi, off);
      argmax_pick(mv, mi, v2, i2);
    }
    const int c0 = q * 4;
    const float t0 = gv.x + gm0 + (mi == c0 ? gm1 : 0.f), t1 = gv.y + gm0 + (mi == c0 + 1 ? gm1 : 0.f);
    const float t2 = gv.z + gm0 + (mi == c0 + 2 ? gm1 : 0.f), t3 = gv.w + gm0 + (mi == c0 + 3 ? gm1 : 0.f);
    *(float4*)(g_o + i * 32 + q * 4) = make_float4(t0 * cav.x, t1 * cav.y, t2 * cav.z, t3 * cav.w);
    acc.x += t0 * ov.x;
    acc.y += t1 * ov.y;
    acc.z += t2 * ov.z;
    acc.w += t3 * ov.w;
  }
  sm[pl][q * 4] = acc.x;
  sm[pl][q * 4 + 1] = acc.y;
  sm[pl][q * 4 + 2] = acc.z;
  sm[pl][q * 4 + 3] = acc.w;
  __syncthreads();
  if (threadIdx.x < 32) {
    float t = 0.f;
    for (int k = 0; k < 32; ++k) t += sm[k][threadIdx.x];
    part[((size_t)b * gridDim.x + blockIdx.x) * 32 + threadIdx.x] = t;
  }
}

__global__ __launch_bounds__(256) void fam_ca_fin_kernel(const float* __restrict__ part, int chunks, int n,
                                                         float* __restrict__ g_ca) {
  __shared__ float red[256];
  const int j = blockIdx.x;  // j = b * 32 + c: one block per output, fixed-order tree
  const int b = j >> 5, c = j & 31;
  float t = 0.f;
  for (int k = threadIdx.x; k < chunks; k += 256) t += part[((size_t)b * chunks + k) * 32 + c];
  red[threadIdx.x] = t;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) g_ca[j] = red[0];
}

__global__ void fam_pool_bwd_kernel(float* g_o, const float* __restrict__ g_pool, const float* __restrict__ o, int B,
                                    int HW, int C) {
  const long long n = (long long)B * HW * C;
  GSTRIDE(i, n) {
    const int c = (int)(i % C);
    const int b = (int)(i / ((long long)HW * C));
    const float v = g_o[i] + g_pool[(size_t)b * C + c] / (float)HW;
    g_o[i] = o[i] > 0.f ? v : 0.f;
  }
}

// the same, 4 channels per thread (the channels of a thread fixed: C / 4
// divides 256), 32-bit offsets (host-checked), and optionally the compact fp16
// copy g16 of the result (the fusion conv's autocast gradient operand)
__global__ __launch_bounds__(256) void fam_pool_bwd4_kernel(float* g_o, const float* __restrict__ g_pool,
                                                            const float* __restrict__ o, int M, int HW, int C,
                                                            half_t* __restrict__ g16) {
  const int C4 = C / 4, c = (threadIdx.x % C4) * 4, rpb = 256 / C4;
  for (int m = blockIdx.x * rpb + threadIdx.x / C4; m < M; m += gridDim.x * rpb) {
    const int b = m / HW;
    const int off = m * C + c;
    const float4 gv = *(const float4*)(g_o + off), ov = *(const float4*)(o + off);
    const float4 pv = *(const float4*)(g_pool + b * C + c);
    float4 r;
    // g_pool / HW as the scalar kernel: a division per element
    r.x = ov.x > 0.f ? gv.x + pv.x / (float)HW : 0.f;
    r.y = ov.y > 0.f ? gv.y + pv.y / (float)HW : 0.f;
    r.z = ov.z > 0.f ? gv.z + pv.z / (float)HW : 0.f;
    r.w = ov.w > 0.f ? gv.w + pv.w / (float)HW : 0.f;
    *(float4*)(g_o + off) = r;
    if (g16) {
      typedef _Float16 h4 __attribute__((ext_vector_type(4)));
      *(h4*)(g16 + off) = h4{(half_t)r.x, (half_t)r.y, (half_t)r.z, (half_t)r.w};
    }
  }
}

// ---------------------------------------------------------------------------
// network tail
// ---------------------------------------------------------------------------
__global__ void head_fwd_kernel(const float* __restrict__ x, const float* __restrict__ r, float* __restrict__ illu,
                                int B, int HW) {
  const long long n = (long long)B * HW;
  GSTRIDE(i, n) {
    const int b = (int)(i / HW), p = (int)(i - (long long)b * HW);
    const float* xb = x + (size_t)b * 3 * HW + p;
    const float z = (xb[0] + xb[HW] + xb[2 * HW]) / 3.f + r[i];
    illu[i] = 1.f / (1.f + expf(-z));
  }
}

__global__ void retinex_fwd_kernel(const float* __restrict__ x, const float* __restrict__ illu,
                                   const float* __restrict__ o, float* __restrict__ e, float* __restrict__ refl,
                                   float* __restrict__ enh, int B, int HW) {
  const long long n = (long long)B * HW;
  GSTRIDE(i, n) {
    const int b = (int)(i / HW), p = (int)(i - (long long)b * HW);
    const float den = illu[i] + 1e-6f;
    for (int c = 0; c < 3; ++c) {
      const size_t k = ((size_t)b * 3 + c) * HW + p;
      const float ev = 1.f / (1.f + expf(-o[i * 3 + c]));
      const float rv = x[k] / den;
      e[i * 3 + c] = ev;
      refl[k] = rv;
      enh[k] = rv * ev + (1.f - rv) * (ev * ev);
    }
  }
}

__global__ void retinex_bwd_kernel(const float* __restrict__ x, const float* __restrict__ illu,
                                   const float* __restrict__ e, const float* __restrict__ refl,
                                   const float* __restrict__ g_enh, const float* __restrict__ g_refl,
                                   const float* __restrict__ g_illu, float* __restrict__ g_o, float* __restrict__ g_r,
                                   int B, int HW) {
  const long long n = (long long)B * HW;
  GSTRIDE(i, n) {
    const int b = (int)(i / HW), p = (int)(i - (long long)b * HW);
    const float il = illu[i];
    const float den = il + 1e-6f;
    float gi = g_illu ? g_illu[i] : 0.f;
    for (int c = 0; c < 3; ++c) {
      const size_t k = ((size_t)b * 3 + c) * HW + p;
      const float ev = e[i * 3 + c], rv = refl[k], ge = g_enh[k];
      // enh = r*e + (1-r)*e^2
      const float gev = ge * (rv + 2.f * ev * (1.f - rv));
      const float grv = ge * (ev - ev * ev) + (g_refl ? g_refl[k] : 0.f);
      g_o[i * 3 + c] = gev * ev * (1.f - ev);
      // r = x / (illu + 1e-6)
      gi -= grv * x[k] / (den * den);
    }
    g_r[i] = gi * il * (1.f - il);
  }
}

// multi_scale_enhance's combine with a caller-given reflectance
// (models/model.py:439-443): e = sigmoid(o), enh = refl*e + (1-refl)*e^2; the
// backward writes dL/do (NHWC, through the sigmoid) and dL/drefl (NCHW)
__global__ void enhance_fwd_kernel(const float* __restrict__ refl, const float* __restrict__ o, float* __restrict__ e,
                                   float* __restrict__ enh, int B, int HW) {
  const long long n = (long long)B * HW;
  GSTRIDE(i, n) {
    const int b = (int)(i / HW), p = (int)(i - (long long)b * HW);
    for (int c = 0; c < 3; ++c) {
      const size_t k = ((size_t)b * 3 + c) * HW + p;
      const float ev = 1.f / (1.f + expf(-o[i * 3 + c]));
      const float rv = refl[k];
      e[i * 3 + c] = ev;
      enh[k] = rv * ev + (1.f - rv) * (ev * ev);
    }
  }
}

__global__ void enhance_bwd_kernel(const float* __restrict__ e, const float* __restrict__ refl,
                                   const float* __restrict__ g_enh, float* __restrict__ g_o,
                                   float* __restrict__ g_refl, int B, int HW) {
  const long long n = (long long)B * HW;
  GSTRIDE(i, n) {
    const int b = (int)(i / HW), p = (int)(i - (long long)b * HW);
    for (int c = 0; c < 3; ++c) {
      const size_t k = ((size_t)b * 3 + c) * HW + p;
      const float ev = e[i * 3 + c], rv = refl[k], ge = g_enh[k];
      g_o[i * 3 + c] = ge * (rv + 2.f * ev * (1.f - rv)) * ev * (1.f - ev);
      if (g_refl) g_refl[k] = ge * (ev - ev * ev);
    }
  }
}

}  // namespace upr

using namespace upr;

extern "C" {

int upr_t_fam_ca_apply(const float* o, const float* ca, int B, int HW, int C, float* o2, float* m, void* stream) {
  if (!o || !ca || !o2 || !m) return UPR_ERR_ARG;
  if (C == 32 && al16(o) && al16(ca) && al16(o2)) {
    hipLaunchKernelGGL(fam_ca_apply32_kernel, dim3(grid_for((long long)B * HW * 8)), dim3(256), 0, ST(stream), o, ca,
                       B, HW, o2, m);
    LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(fam_ca_apply_kernel, dim3(grid_for((long long)B * HW)), dim3(256), 0, ST(stream), o, ca, B, HW,
                     C, o2, m);
  LAUNCH_CHECK();
}

int upr_t_fam_sa_apply(const float* o2, const float* s_pre, int B, int HW, int C, float* sa, float* out,
                       void* stream) {
  if (!o2 || !s_pre || !sa || !out) return UPR_ERR_ARG;
  if (C == 32 && al16(o2) && al16(out)) {
    hipLaunchKernelGGL(fam_sa_apply32_kernel, dim3(grid_for((long long)B * HW * 8)), dim3(256), 0, ST(stream), o2,
                       s_pre, B, HW, sa, out);
    LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(fam_sa_apply_kernel, dim3(grid_for((long long)B * HW)), dim3(256), 0, ST(stream), o2, s_pre, B,
                     HW, C, sa, out);
  LAUNCH_CHECK();
}

int upr_t_fam_sa_bwd_cs(const float* g, int g_cs, const float* o2, const float* sa, int B, int HW, int C,
                        float* g_o2, float* g_spre, void* stream) {
  if (!g || !o2 || !sa || !g_o2 || !g_spre || g_cs < C) return UPR_ERR_ARG;
  if (C == 32 && g_cs % 4 == 0 && al16(g) && al16(o2) && al16(g_o2)) {
    hipLaunchKernelGGL(fam_sa_bwd32_kernel, dim3(grid_for((long long)B * HW * 8)), dim3(256), 0, ST(stream), g, g_cs,
                       o2, sa, B, HW, g_o2, g_spre);
    LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(fam_sa_bwd_kernel, dim3(grid_for((long long)B * HW)), dim3(256), 0, ST(stream), g, g_cs, o2, sa,
                     B, HW, C, g_o2, g_spre);
  LAUNCH_CHECK();
}

int upr_t_fam_sa_bwd(const float* g, const float* o2, const float* sa, int B, int HW, int C, float* g_o2,
                     float* g_spre, void* stream) {
  return upr_t_fam_sa_bwd_cs(g, C, o2, sa, B, HW, C, g_o2, g_spre, stream);
}

int upr_t_fam_ca_bwd(const float* g_o2, const float* g_m, const float* o, const float* o2, const float* ca, int B,
                     int HW, int C, float* g_o, float* g_ca, void* stream) {
  if (!g_o2 || !g_m || !o || !o2 || !ca || !g_o || !g_ca || C > 32) return UPR_ERR_ARG;
  if (C == 32 && al16(g_o2) && al16(o) && al16(o2) && al16(ca) && al16(g_o) && B > 0 && HW > 0) {
    hipStream_t st = ST(stream);
    int chunks = HW / 1024;
    chunks = chunks < 1 ? 1 : (chunks > 256 ? 256 : chunks);
    float* part = nullptr;
    part = (float*)scratch(kSlotPart, sizeof(float) * 32 * B * chunks, st);
    if (!part) return (int)hipErrorOutOfMemory;
    hipLaunchKernelGGL(fam_ca_bwd32_kernel, dim3(chunks, B), dim3(256), 0, st, g_o2, g_m, o, o2, ca, HW, g_o, part);
    hipLaunchKernelGGL(fam_ca_fin_kernel, dim3(B * 32), dim3(256), 0, st, (const float*)part, chunks, B * 32, g_ca);
    UPR_CHECK_HIP(hipGetLastError());
    return UPR_OK;
  }
  UPR_CHECK_HIP(hipMemsetAsync(g_ca, 0, sizeof(float) * B * C, ST(stream)));
  int chunks = HW / 4096;
  chunks = chunks < 1 ? 1 : (chunks > 256 ? 256 : chunks);
  hipLaunchKernelGGL(fam_ca_bwd_kernel, dim3(chunks, B), dim3(256), 0, ST(stream), g_o2, g_m, o, o2, ca, HW, C, g_o,
                     g_ca);
  LAUNCH_CHECK();
}

int upr_t_fam_pool_bwd16(float* g_o, const float* g_pool, const float* o, int B, int HW, int C, void* g16,
                         void* stream) {
  if (!g_o || !g_pool || !o || B <= 0 || HW <= 0 || C <= 0) return UPR_ERR_ARG;
  const long long n = (long long)B * HW * C;
  if (C % 4 == 0 && 256 % (C / 4) == 0 && n < (1LL << 31) && al16(g_o) && al16(g_pool) && al16(o) &&
      (uintptr_t)g16 % 8 == 0) {
    const long long M = (long long)B * HW;
    hipLaunchKernelGGL(fam_pool_bwd4_kernel, dim3(grid_for(M * (C / 4))), dim3(256), 0, ST(stream), g_o, g_pool, o,
                       (int)M, HW, C, (half_t*)g16);
    LAUNCH_CHECK();
  }
  if (g16) return UPR_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(fam_pool_bwd_kernel, dim3(grid_for(n)), dim3(256), 0, ST(stream), g_o, g_pool, o, B, HW, C);
  LAUNCH_CHECK();
}

int upr_t_fam_pool_bwd(float* g_o, const float* g_pool, const float* o, int B, int HW, int C, void* stream) {
  return upr_t_fam_pool_bwd16(g_o, g_pool, o, B, HW, C, nullptr, stream);
}

int upr_t_head_fwd(const float* x, const float* r, float* illu, int B, int H, int W, void* stream) {
  if (!x || !r || !illu) return UPR_ERR_ARG;
  hipLaunchKernelGGL(head_fwd_kernel, dim3(grid_for((long long)B * H * W)), dim3(256), 0, ST(stream), x, r, illu, B,
                     H * W);
  LAUNCH_CHECK();
}

int upr_t_retinex_fwd(const float* x, const float* illu, const float* o, float* e, float* refl, float* enh, int B,
                      int H, int W, void* stream) {
  if (!x || !illu || !o || !e || !refl || !enh) return UPR_ERR_ARG;
  hipLaunchKernelGGL(retinex_fwd_kernel, dim3(grid_for((long long)B * H * W)), dim3(256), 0, ST(stream), x, illu, o,
                     e, refl, enh, B, H * W);
  LAUNCH_CHECK();
}

int upr_t_retinex_bwd(const float* x, const float* illu, const float* e, const float* refl, const float* g_enh,
                      const float* g_refl, const float* g_illu, float* g_o, float* g_r, int B, int H, int W,
                      void* stream) {
  if (!x || !illu || !e || !refl || !g_enh || !g_o || !g_r) return UPR_ERR_ARG;
  hipLaunchKernelGGL(retinex_bwd_kernel, dim3(grid_for((long long)B * H * W)), dim3(256), 0, ST(stream), x, illu, e,
                     refl, g_enh, g_refl, g_illu, g_o, g_r, B, H * W);
  LAUNCH_CHECK();
}

int upr_t_enhance_fwd(const float* refl, const float* o, float* e, float* enh, int B, int H, int W, void* stream) {
  if (!refl || !o || !e || !enh) return UPR_ERR_ARG;
  hipLaunchKernelGGL(enhance_fwd_kernel, dim3(grid_for((long long)B * H * W)), dim3(256), 0, ST(stream), refl, o, e,
                     enh, B, H * W);
  LAUNCH_CHECK();
}

int upr_t_enhance_bwd(const float* e, const float* refl, const float* g_enh, float* g_o, float* g_refl, int B, int H,
                      int W, void* stream) {
  if (!e || !refl || !g_enh || !g_o) return UPR_ERR_ARG;
  hipLaunchKernelGGL(enhance_bwd_kernel, dim3(grid_for((long long)B * H * W)), dim3(256), 0, ST(stream), e, refl,
                     g_enh, g_o, g_refl, B, H * W);
  LAUNCH_CHECK();
}

}  // extern "C"
