// Shared by the training units (train_conv.hip, train_bn.hip,
// train_pointwise.hip, train_resample.hip, train_loss.hip, train_fam.hip,
// train_optim.hip, train_small.hip, train_wgrad.hip): the strided-view kernel
// arguments, launch helpers, vector typedefs, the device helpers two units
// use, and the prototypes of every function one training unit calls in
// another.
//
// Layout: activations are addressed through UprView strides (NCHW inputs,
// NHWC activations, channel slices of concat buffers).  Everything computes in
// fp32; per-channel / per-image reductions accumulate in fp64 (block partials
// in registers + LDS, one fp64 atomic per block and channel).
#pragma once
#include <cstdint>

#include "upr_common.h"
#include "../../include/upr.h"
#include "../../include/upr_train.h"

namespace upr {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

struct V {
  float* d;
  long long sb, sh, sw, sc;
  __device__ __forceinline__ long long at(int b, int y, int x, int c) const {
    return b * sb + y * sh + x * sw + c * sc;
  }
};

static V mkv(const UprView* u) {
  V v;
  v.d = (float*)u->data;
  v.sb = u->sb; v.sh = u->sh; v.sw = u->sw; v.sc = u->sc;
  return v;
}

// channel-contiguous view with 32-bit strides: the 4-channels-per-thread
// resampling / copy kernels (the generic V kernels' 64-bit div/mod per element
// run below 1 TB/s)
struct V4 {
  float* d;
  int sb, sh, sw;
  __device__ __forceinline__ float* at(int b, int y, int x, int c) const { return d + b * sb + y * sh + x * sw + c; }
};

// usable as a V4 over [B, H, W, C]: unit channel stride, C and the strides
// multiples of 4, 16-byte aligned, every offset below 2^31
static bool vec4_view_ok(const UprView* v, int B, int H, int W, int C) {
  if (v->sc != 1 || C % 4 || (uintptr_t)v->data % 16 || v->sw % 4 || v->sh % 4 || v->sb % 4) return false;
  if ((long long)B * H * W * C >= (1LL << 31)) return false;
  const long long ext = (long long)(B - 1) * v->sb + (long long)(H - 1) * v->sh + (long long)(W - 1) * v->sw + C;
  return ext < (1LL << 31) && v->sb < (1LL << 31) && v->sh < (1LL << 31) && v->sw < (1LL << 31);
}

// 4 consecutive channels as floats, from fp32 or an fp16 copy
__device__ __forceinline__ float4 ld4f(const float* p) { return *(const float4*)p; }
__device__ __forceinline__ float4 ld4f(const half_t* p) {
  typedef _Float16 h4 __attribute__((ext_vector_type(4)));
  const h4 v = *(const h4*)p;
  return make_float4((float)v[0], (float)v[1], (float)v[2], (float)v[3]);
}

// thread i of a V4 kernel over [B][H][W][CV * 4] -> pixel (b, y, x) and the first of its 4 channels
__device__ __forceinline__ void dec4(int i, int CV, int W, int H, int& b, int& y, int& x, int& c) {
  c = (i % CV) * 4;
  int r = i / CV;
  x = r % W;
  r /= W;
  y = r % H;
  b = r / H;
}

// d16 (nullable): fp16 copy of the result at d16[pixel * cs16 + c] (pixel = (b*H + y)*W + x)
__device__ __forceinline__ void store16(half_t* d16, int cs16, int pix, int c, float4 v) {
  typedef _Float16 h4 __attribute__((ext_vector_type(4)));
  *(h4*)(d16 + (size_t)pix * cs16 + c) = h4{(half_t)v.x, (half_t)v.y, (half_t)v.z, (half_t)v.w};
}

static V4 mkv4(const UprView* u) {
  V4 v;
  v.d = (float*)u->data;
  v.sb = (int)u->sb; v.sh = (int)u->sh; v.sw = (int)u->sw;
  return v;
}

static inline int grid_for(long long n, int per = 256, int cap = 65536) {
  long long g = (n + per - 1) / per;
  if (g < 1) g = 1;
  return (int)(g > cap ? cap : g);
}

#define GSTRIDE(i, n) for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < (n); \
                           i += (long long)gridDim.x * blockDim.x)

#define LAUNCH_CHECK() return (int)hipGetLastError()

#define ST(s) ((hipStream_t)(s))

static bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

template <int NV>
__device__ __forceinline__ void block_sum_atomic(double (&v)[NV], double* dst[NV]) {
  __shared__ double sm[NV][256];
#pragma unroll
  for (int k = 0; k < NV; ++k) sm[k][threadIdx.x] = v[k];
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (threadIdx.x < s) {
#pragma unroll
      for (int k = 0; k < NV; ++k) sm[k][threadIdx.x] += sm[k][threadIdx.x + s];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < NV; ++k)
      if (dst[k]) atomicAdd(dst[k], sm[k][0]);
  }
  __syncthreads();
}

// train_small.hip: pixel-tiled / MFMA forms of the small-channel convs
int small_conv_fwd(const UprView* xv, int B, int H, int W, int Cin, const float* w, const float* bias, int Cout,
                   int kh, int kw, int stride, int pad, int dil, const UprView* yv, int Ho, int Wo, int relu,
                   int accumulate, hipStream_t st, void* y16 = nullptr, int skip32 = 0);
int small_stem_wgrad_relu16(const UprView* xv, const float* dy, const void* y16, int B, int H, int W, float* dw,
                            float* dbias, hipStream_t st);
int small_conv_dgrad(const UprView* dyv, int Ho, int Wo, const float* w, int B, int H, int W, int Cin, int Cout,
                     int kh, int kw, int stride, int pad, int dil, const UprView* dxv, int accumulate, hipStream_t st);
int small_conv_dgrad_c3_16(const void* dy16, int B, int H, int W, const float* w, int Cout, const UprView* dxv,
                           int accumulate, hipStream_t st);
int small_conv_wgrad(const UprView* xv, const UprView* dyv, int B, int H, int W, int Cin, int Ho, int Wo, int Cout,
                     int kh, int kw, int stride, int pad, int dil, float* dw, float* dbias, hipStream_t st,
                     const UprView* ymask = nullptr);
// dw[co][k] (k < KC) and dbias[co] (k == KC; skipped when NULL) += the sum over blocks of part[block][co][KC + 1],
// in block order (small_wgrad_fin_kernel)
int small_wgrad_finish(const float* part, int blocks, int Cout, int KC, float* dw, float* dbias, hipStream_t st);
// train_wgrad.hip: split-K GEMM weight gradient (train_conv.hip's conv_wgrad_kernel takes the shapes it does not)
int wgrad_gemm(const float* x, int B, int H, int W, int Cin, int x_cs, int x_coff, const float* dy, int Ho, int Wo,
               int Cout, int dy_cs, int dy_coff, int kh, int kw, int stride, int pad, int dil, float* dwp,
               hipStream_t st, int torch_ci = 0);
int wgrad16_gemm(const void* x16, int B, int H, int W, int Cin, const float* dy, int Ho, int Wo, int Cout, int dy_cs,
                 int dy_coff, int kh, int kw, int stride, int pad, int dil, float* dwp, hipStream_t st,
                 int torch_ci = 0, const void* dy16 = nullptr);
// the calling thread's record for upr_t_conv_wgrad_ran: an entry clears it (kernel UPR_WGRAD_NONE),
// the launcher that queues a weight-gradient kernel fills it in
void wgrad_ran_set(int kernel, int t0 = 0, int t1 = 0, int t2 = 0, int splits = 0, int dy16 = 0);
const UprWgradRan& wgrad_ran();

}  // namespace upr
