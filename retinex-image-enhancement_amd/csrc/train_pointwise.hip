// Elementwise training kernels for gfx950: ReLU masks, strided copies,
// sigmoid / dropout / add / scale, and the sums and copies that also write
// their fp16 copy.
// Entries: include/upr_train.h; layout and precision: train_common.h.
#include <cmath>

#include "train_common.h"

namespace upr {

// ---------------------------------------------------------------------------
// elementwise
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void relu_mask4_kernel(float* g, int g_cs, int g_coff, const float* __restrict__ y,
                                                         int y_cs, int y_coff, int M, int C) {
  const int C4 = C / 4;
  if (256 % C4 == 0) {  // fixed channels per thread (see bn_apply4_kernel)
    const int c = (threadIdx.x % C4) * 4, rpb = 256 / C4;
    for (int m = blockIdx.x * rpb + threadIdx.x / C4; m < M; m += gridDim.x * rpb) {
      const float4 yv = *(const float4*)(y + (size_t)m * y_cs + y_coff + c);
      float4* gp = (float4*)(g + (size_t)m * g_cs + g_coff + c);
      float4 gv = *gp;
      if (!(yv.x > 0.f)) gv.x = 0.f;
      if (!(yv.y > 0.f)) gv.y = 0.f;
      if (!(yv.z > 0.f)) gv.z = 0.f;
      if (!(yv.w > 0.f)) gv.w = 0.f;
      *gp = gv;
    }
    return;
  }
  const long long n = (long long)M * C4;
  GSTRIDE(i, n) {
    const int c = (int)(i % C4) * 4;
    const long long m = i / C4;
    const float4 yv = *(const float4*)(y + m * y_cs + y_coff + c);
    float4* gp = (float4*)(g + m * g_cs + g_coff + c);
    float4 gv = *gp;
    if (!(yv.x > 0.f)) gv.x = 0.f;
    if (!(yv.y > 0.f)) gv.y = 0.f;
    if (!(yv.z > 0.f)) gv.z = 0.f;
    if (!(yv.w > 0.f)) gv.w = 0.f;
    *gp = gv;
  }
}

// the mask fused with the fp16 copy of the masked gradient (the autocast
// dgrad operand, trainers/train.py:72): g16[m][c] = half(g masked), g itself
// rewritten only with write32 (a frozen conv's gradient has no fp32 reader)
// TY = half_t: the mask from the activation's fp16 copy (the autocast VGG
// activations are fp16 only; (half)y > 0 <=> y > 0 for their fp16-exact values)
template <typename TY = float>
__global__ __launch_bounds__(256) void relu_mask16_kernel(float* g, int g_cs, int g_coff, const TY* __restrict__ y,
                                                          int y_cs, int y_coff, int M, int C4,
                                                          half_t* __restrict__ g16, int write32) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= M * C4) return;
  const int c = (i % C4) * 4, m = i / C4;
  const float4 yv = ld4f(y + (size_t)m * y_cs + y_coff + c);
  float4* gp = (float4*)(g + (size_t)m * g_cs + g_coff + c);
  float4 gv = *gp;
  if (!(yv.x > 0.f)) gv.x = 0.f;
  if (!(yv.y > 0.f)) gv.y = 0.f;
  if (!(yv.z > 0.f)) gv.z = 0.f;
  if (!(yv.w > 0.f)) gv.w = 0.f;
  if (write32) *gp = gv;
  typedef _Float16 h4 __attribute__((ext_vector_type(4)));
  *(h4*)(g16 + (size_t)i * 4) = h4{(half_t)gv.x, (half_t)gv.y, (half_t)gv.z, (half_t)gv.w};
}

__global__ void relu_mask_kernel(float* g, int g_cs, int g_coff, const float* __restrict__ y, int y_cs, int y_coff,
                                 int M, int C) {
  const long long n = (long long)M * C;
  GSTRIDE(i, n) {
    const int c = (int)(i % C);
    const long long m = i / C;
    if (!(y[m * y_cs + y_coff + c] > 0.f)) g[m * g_cs + g_coff + c] = 0.f;
  }
}

__global__ void copy_kernel(V s, V d, int B, int H, int W, int C, int accum) {
  const long long n = (long long)B * H * W * C;
  GSTRIDE(i, n) {
    const int c = (int)(i % C);
    long long r = i / C;
    const int x = (int)(r % W); r /= W;
    const int y = (int)(r % H);
    const int b = (int)(r / H);
    const float v = s.d[s.at(b, y, x, c)];
    float* o = d.d + d.at(b, y, x, c);
    *o = accum ? *o + v : v;
  }
}

__global__ __launch_bounds__(256) void copy4_kernel(V4 s, V4 d, int H, int W, int CV, int n, int accum,
                                                    half_t* __restrict__ d16, int cs16) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  int b, y, x, c;
  dec4(i, CV, W, H, b, y, x, c);
  float4 v = *(const float4*)s.at(b, y, x, c);
  float4* o = (float4*)d.at(b, y, x, c);
  if (accum == 1) {
    const float4 u = *o;
    v = make_float4(u.x + v.x, u.y + v.y, u.z + v.z, u.w + v.w);
  }
  if (accum != 2) *o = v;  // 2: the fp16 copy only
  if (d16) store16(d16, cs16, i / CV, c, v);
}

__device__ __forceinline__ float hash_uniform(unsigned long long seed, unsigned long long i) {
  // splitmix64 of (seed, index) -> [0, 1)
  unsigned long long z = seed + 0x9E3779B97F4A7C15ull * (i + 1);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z ^= z >> 31;
  return (float)(z >> 40) * (1.0f / 16777216.0f);
}

__global__ void pointwise_kernel(const float* a, const float* b, float* out, long long n, int op,
                                 const uint8_t* __restrict__ mask_in, uint8_t* __restrict__ mask_out, float p,
                                 unsigned long long seed) {
  GSTRIDE(i, n) {
    const float av = a[i];
    float v;
    switch (op) {
      case 0: v = 1.f / (1.f + expf(-av)); break;
      case 1: { const float s = b[i]; v = av * s * (1.f - s); } break;
      case 2: {
        const uint8_t m = hash_uniform(seed, (unsigned long long)i) >= p ? 1 : 0;
        mask_out[i] = m;
        v = m ? av * (1.f / (1.f - p)) : 0.f;
      } break;
      case 3: v = mask_in[i] ? av * (1.f / (1.f - p)) : 0.f; break;
      case 4: v = av + b[i]; break;
      default: v = av * b[0]; break;
    }
    out[i] = v;
  }
}

// out = a + b with its fp16 copy (a residual / skip sum feeding an autocast conv)
__global__ __launch_bounds__(256) void add16_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                    float* __restrict__ out, half_t* __restrict__ out16, int n4) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n4) return;
  const float4 u = ((const float4*)a)[i], v = ((const float4*)b)[i];
  const float4 r = make_float4(u.x + v.x, u.y + v.y, u.z + v.z, u.w + v.w);
  ((float4*)out)[i] = r;
  typedef _Float16 h4 __attribute__((ext_vector_type(4)));
  ((h4*)out16)[i] = h4{(half_t)r.x, (half_t)r.y, (half_t)r.z, (half_t)r.w};
}

}  // namespace upr

using namespace upr;

extern "C" {

int upr_t_zero(void* p, size_t bytes, void* stream) {
  if (!p && bytes) return UPR_ERR_ARG;
  if (!bytes) return UPR_OK;
  return (int)hipMemsetAsync(p, 0, bytes, ST(stream));
}

int upr_t_relu_mask(float* g, int g_cs, int g_coff, const float* y, int y_cs, int y_coff, int M, int C,
                    void* stream) {
  if (!g || !y) return UPR_ERR_ARG;
  if (C % 4 == 0 && g_cs % 4 == 0 && g_coff % 4 == 0 && y_cs % 4 == 0 && y_coff % 4 == 0 && ((uintptr_t)g & 15) == 0 &&
      ((uintptr_t)y & 15) == 0) {
    const long long n4 = (long long)M * (C / 4);
    hipLaunchKernelGGL(relu_mask4_kernel, dim3(grid_for(n4)), dim3(256), 0, ST(stream), g, g_cs, g_coff, y, y_cs,
                       y_coff, M, C);
    LAUNCH_CHECK();
  }
  const long long n = (long long)M * C;
  hipLaunchKernelGGL(relu_mask_kernel, dim3(grid_for(n)), dim3(256), 0, ST(stream), g, g_cs, g_coff, y, y_cs, y_coff,
                     M, C);
  LAUNCH_CHECK();
}

int upr_t_relu_mask16(float* g, int g_cs, int g_coff, const float* y, int y_cs, int y_coff, int M, int C, void* g16,
                      int write32, void* stream) {
  if (!g || !y || !g16) return UPR_ERR_ARG;
  if (C % 4 || g_cs % 4 || g_coff % 4 || y_cs % 4 || y_coff % 4 || ((uintptr_t)g & 15) || ((uintptr_t)y & 15) ||
      ((uintptr_t)g16 & 7) || (long long)M * C >= (1LL << 31))
    return UPR_ERR_UNSUPPORTED;
  const int n = M * (C / 4);
  if (n == 0) return UPR_OK;
  hipLaunchKernelGGL(relu_mask16_kernel<float>, dim3((n + 255) / 256), dim3(256), 0, ST(stream), g, g_cs, g_coff, y,
                     y_cs, y_coff, M, C / 4, (half_t*)g16, write32);
  LAUNCH_CHECK();
}

int upr_t_relu_mask16h(float* g, int g_cs, int g_coff, const void* y16, int y16_cs, int M, int C, void* g16,
                       int write32, void* stream) {
  if (!g || !y16 || !g16) return UPR_ERR_ARG;
  if (C % 4 || g_cs % 4 || g_coff % 4 || y16_cs % 4 || ((uintptr_t)g & 15) || ((uintptr_t)y16 & 7) ||
      ((uintptr_t)g16 & 7) || (long long)M * C >= (1LL << 31))
    return UPR_ERR_UNSUPPORTED;
  const int n = M * (C / 4);
  if (n == 0) return UPR_OK;
  hipLaunchKernelGGL(relu_mask16_kernel<half_t>, dim3((n + 255) / 256), dim3(256), 0, ST(stream), g, g_cs, g_coff,
                     (const half_t*)y16, y16_cs, 0, M, C / 4, (half_t*)g16, write32);
  LAUNCH_CHECK();
}

int upr_t_copy(const UprView* src, const UprView* dst, int B, int H, int W, int C, int accumulate, void* stream) {
  if (!src || !dst || !src->data || !dst->data) return UPR_ERR_ARG;
  const long long n = (long long)B * H * W * C;
  if (n == 0) return UPR_OK;
  if (vec4_view_ok(src, B, H, W, C) && vec4_view_ok(dst, B, H, W, C)) {
    const int nv = (int)(n / 4);
    hipLaunchKernelGGL(copy4_kernel, dim3((nv + 255) / 256), dim3(256), 0, ST(stream), mkv4(src), mkv4(dst), H, W,
                       C / 4, nv, accumulate, (half_t*)nullptr, 0);
    LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(copy_kernel, dim3(grid_for(n)), dim3(256), 0, ST(stream), mkv(src), mkv(dst), B, H, W, C,
                     accumulate);
  LAUNCH_CHECK();
}

int upr_t_pointwise(const float* a, const float* b, float* out, size_t n, int op, const uint8_t* mask_in,
                    uint8_t* mask_out, float p, uint64_t seed, void* stream) {
  if (!a || !out || op < 0 || op > 5) return UPR_ERR_ARG;
  if ((op == 1 || op == 4 || op == 5) && !b) return UPR_ERR_ARG;
  if ((op == 2 && !mask_out) || (op == 3 && !mask_in)) return UPR_ERR_ARG;
  if (n == 0) return UPR_OK;
  hipLaunchKernelGGL(pointwise_kernel, dim3(grid_for((long long)n)), dim3(256), 0, ST(stream), a, b, out,
                     (long long)n, op, mask_in, mask_out, p, (unsigned long long)seed);
  LAUNCH_CHECK();
}

int upr_t_copy16(const UprView* src, const UprView* dst, int B, int H, int W, int C, int accumulate, void* dst16,
                 int dst16_cs, void* stream) {
  if (!src || !dst || !src->data || !dst->data || !dst16 || accumulate < 0 || accumulate > 2) return UPR_ERR_ARG;
  const long long n = (long long)B * H * W * C;
  if (n == 0) return UPR_OK;
  if (!vec4_view_ok(src, B, H, W, C) || !vec4_view_ok(dst, B, H, W, C) || (uintptr_t)dst16 % 8 || dst16_cs % 4 ||
      (long long)B * H * W * dst16_cs >= (1LL << 31))
    return UPR_ERR_UNSUPPORTED;
  const int nv = (int)(n / 4);
  hipLaunchKernelGGL(copy4_kernel, dim3((nv + 255) / 256), dim3(256), 0, ST(stream), mkv4(src), mkv4(dst), H, W, C / 4,
                     nv, accumulate, (half_t*)dst16, dst16_cs);
  LAUNCH_CHECK();
}

int upr_t_add16(const float* a, const float* b, float* out, size_t n, void* out16, void* stream) {
  if (!a || !b || !out || !out16) return UPR_ERR_ARG;
  if (n % 4 || n / 4 >= (1ULL << 31) || ((uintptr_t)a | (uintptr_t)b | (uintptr_t)out) % 16 || (uintptr_t)out16 % 8)
    return UPR_ERR_UNSUPPORTED;
  if (n == 0) return UPR_OK;
  const int n4 = (int)(n / 4);
  hipLaunchKernelGGL(add16_kernel, dim3((n4 + 255) / 256), dim3(256), 0, ST(stream), a, b, out, (half_t*)out16, n4);
  LAUNCH_CHECK();
}

}  // extern "C"
