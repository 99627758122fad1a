// Convolution training kernels for gfx950: the direct small-channel conv
// (forward / dgrad / wgrad), the MFMA weight gradient, weight packing and
// gradient unpacking, the zero-upsampled stride-2 gradient and the autocast
// casts.  The conv entries dispatch to train_small.hip, train_wgrad.hip and
// the forward library's MFMA convs where those take the shape.
// Entries: include/upr_train.h; layout and precision: train_common.h.
#include <cmath>
#include <cstring>

#include "train_common.h"

namespace upr {

// ---------------------------------------------------------------------------
// Direct convolution (small channel counts): forward / dgrad / wgrad
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void conv_direct_kernel(V x, int B, int H, int W, int Cin, const float* __restrict__ w,
                                                          const float* __restrict__ bias, int Cout, int kh, int kw,
                                                          int s, int p, int d, V y, int Ho, int Wo, int relu,
                                                          int accum) {
  const long long n = (long long)B * Ho * Wo * Cout;
  GSTRIDE(i, n) {
    const int co = (int)(i % Cout);
    long long r = i / Cout;
    const int ox = (int)(r % Wo); r /= Wo;
    const int oy = (int)(r % Ho);
    const int b = (int)(r / Ho);
    float a = bias ? bias[co] : 0.f;
    const float* wc = w + (size_t)co * Cin * kh * kw;
    for (int ci = 0; ci < Cin; ++ci) {
      for (int ky = 0; ky < kh; ++ky) {
        const int iy = oy * s - p + ky * d;
        if (iy < 0 || iy >= H) continue;
        for (int kx = 0; kx < kw; ++kx) {
          const int ix = ox * s - p + kx * d;
          if (ix < 0 || ix >= W) continue;
          a = fmaf(x.d[x.at(b, iy, ix, ci)], wc[(ci * kh + ky) * kw + kx], a);
        }
      }
    }
    float* yp = y.d + y.at(b, oy, ox, co);
    if (accum) a += *yp;
    if (relu) a = fmaxf(a, 0.f);
    *yp = a;
  }
}

// 3-input-channel 3x3 stride-1 dilation-1 form (the input layers 3->32 and
// VGG-19 conv1_1 3->64 at full resolution): compile-time tap loops, the 27
// weights in registers, one base pointer per tap row -- the generic kernel's
// per-access 64-bit four-stride index arithmetic dominated its time
__global__ __launch_bounds__(256) void conv_direct_c3k3_kernel(V x, int B, int H, int W, const float* __restrict__ w,
                                                               const float* __restrict__ bias, int Cout, int p, V y,
                                                               int Ho, int Wo, int relu, int accum) {
  const long long n = (long long)B * Ho * Wo * Cout;
  GSTRIDE(i, n) {
    const int co = (int)(i % Cout);
    long long r = i / Cout;
    const int ox = (int)(r % Wo); r /= Wo;
    const int oy = (int)(r % Ho);
    const int b = (int)(r / Ho);
    const float* wc = w + (size_t)co * 27;
    float a = bias ? bias[co] : 0.f;
    // same accumulation order as conv_direct_kernel: ci outer, then ky, kx
#pragma unroll
    for (int ci = 0; ci < 3; ++ci) {
#pragma unroll
      for (int ky = 0; ky < 3; ++ky) {
        const int iy = oy - p + ky;
        if (iy < 0 || iy >= H) continue;
        const float* row = x.d + b * x.sb + iy * x.sh + ci * x.sc;
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
          const int ix = ox - p + kx;
          if (ix < 0 || ix >= W) continue;
          a = fmaf(row[ix * x.sw], wc[(ci * 3 + ky) * 3 + kx], a);
        }
      }
    }
    float* yp = y.d + y.at(b, oy, ox, co);
    if (accum) a += *yp;
    if (relu) a = fmaxf(a, 0.f);
    *yp = a;
  }
}

__global__ __launch_bounds__(256) void conv_direct_dgrad_kernel(V dy, int Ho, int Wo, const float* __restrict__ w,
                                                                int B, int H, int W, int Cin, int Cout, int kh,
                                                                int kw, int s, int p, int d, V dx, int accum) {
  const long long n = (long long)B * H * W * Cin;
  GSTRIDE(i, n) {
    const int ci = (int)(i % Cin);
    long long r = i / Cin;
    const int ix = (int)(r % W); r /= W;
    const int iy = (int)(r % H);
    const int b = (int)(r / H);
    float a = 0.f;
    for (int ky = 0; ky < kh; ++ky) {
      const int yn = iy + p - ky * d;
      if (yn < 0 || yn % s) continue;
      const int oy = yn / s;
      if (oy >= Ho) continue;
      for (int kx = 0; kx < kw; ++kx) {
        const int xn = ix + p - kx * d;
        if (xn < 0 || xn % s) continue;
        const int ox = xn / s;
        if (ox >= Wo) continue;
        for (int co = 0; co < Cout; ++co)
          a = fmaf(dy.d[dy.at(b, oy, ox, co)], w[(((size_t)co * Cin + ci) * kh + ky) * kw + kx], a);
      }
    }
    float* xp = dx.d + dx.at(b, iy, ix, ci);
    if (accum) a += *xp;
    *xp = a;
  }
}

// Weight gradient of a small conv: a chunk of CH output pixels is staged in
// LDS as dy[CH][Cout] and its im2col rows col[CH][taps*Cin]; each thread owns
// weight entries (co, ci, tap) (+ a bias entry), sums each over the chunk and
// adds the chunk's sum to its running sum.  Blocks loop over chunks
// (grid-stride) and write one partial row each, part[block][co][KC + 1] in
// PyTorch's (ci, ky, kx) order with the bias entry last, which
// small_wgrad_finish adds in block order.  (One fp32 atomic a block and entry
// made up to 1024 additions in arrival order at the full magnitude of the
// sum: 7 ulp on the bias of a 260 x 260 image.)
__global__ __launch_bounds__(256) void conv_direct_wgrad_kernel(V x, V dy, int B, int H, int W, int Cin, int Ho,
                                                                int Wo, int Cout, int kh, int kw, int s, int p,
                                                                int d, int CH, int with_bias,
                                                                float* __restrict__ part) {
  extern __shared__ float sm[];
  const int taps = kh * kw;
  const int KC = taps * Cin;
  float* sdy = sm;              // [CH][Cout]
  float* scol = sm + CH * Cout;  // [CH][KC]
  const long long P = (long long)B * Ho * Wo;
  const int nW = Cout * KC;
  const int nE = nW + (with_bias ? Cout : 0);
  constexpr int MAXE = 16;
  float acc[MAXE];
#pragma unroll
  for (int k = 0; k < MAXE; ++k) acc[k] = 0.f;
  for (long long c0 = (long long)blockIdx.x * CH; c0 < P; c0 += (long long)gridDim.x * CH) {
    __syncthreads();
    for (int t = threadIdx.x; t < CH * Cout; t += blockDim.x) {
      const int pp = t / Cout, co = t - pp * Cout;
      const long long pix = c0 + pp;
      float v = 0.f;
      if (pix < P) {
        const int ox = (int)(pix % Wo);
        const long long r = pix / Wo;
        const int oy = (int)(r % Ho), b = (int)(r / Ho);
        v = dy.d[dy.at(b, oy, ox, co)];
      }
      sdy[t] = v;
    }
    for (int t = threadIdx.x; t < CH * KC; t += blockDim.x) {
      const int pp = t / KC, k = t - pp * KC;
      const int tap = k / Cin, ci = k - tap * Cin;
      const int ky = tap / kw, kx = tap - ky * kw;
      const long long pix = c0 + pp;
      float v = 0.f;
      if (pix < P) {
        const int ox = (int)(pix % Wo);
        const long long r = pix / Wo;
        const int oy = (int)(r % Ho), b = (int)(r / Ho);
        const int iy = oy * s - p + ky * d, ix = ox * s - p + kx * d;
        if (iy >= 0 && iy < H && ix >= 0 && ix < W) v = x.d[x.at(b, iy, ix, ci)];
      }
      scol[t] = v;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < MAXE; ++k) {
      const int e = threadIdx.x + k * 256;
      if (e >= nE) break;
      float a = 0.f;
      if (e < nW) {
        const int co = e / KC, kk = e - co * KC;
        for (int pp = 0; pp < CH; ++pp) a = fmaf(sdy[pp * Cout + co], scol[pp * KC + kk], a);
      } else {
        const int co = e - nW;
        for (int pp = 0; pp < CH; ++pp) a += sdy[pp * Cout + co];
      }
      acc[k] += a;
    }
  }
  float* row = part + (size_t)blockIdx.x * Cout * (KC + 1);
#pragma unroll
  for (int k = 0; k < MAXE; ++k) {
    const int e = threadIdx.x + k * 256;
    if (e >= nE) break;
    if (e < nW) {
      // e = co*KC + tap*Cin + ci -> PyTorch [co][ci][ky][kx]
      const int co = e / KC, kk = e - co * KC;
      const int tap = kk / Cin, ci = kk - tap * Cin;
      row[(size_t)co * (KC + 1) + ci * taps + tap] = acc[k];
    } else {
      row[(size_t)(e - nW) * (KC + 1) + KC] = acc[k];
    }
  }
}

// ---------------------------------------------------------------------------
// MFMA weight gradient (C % 32 == 0): block tile 32 co x 32 ci of one tap,
// 4 waves each summing interleaved groups of 4 pixels with
// v_mfma_f32_16x16x4_f32 (A = dy[p][co], B = x[window(p)][ci], k = pixel).
// ---------------------------------------------------------------------------
constexpr int WG_PPB = 1024;  // pixels per block

__global__ __launch_bounds__(256) void conv_wgrad_kernel(const float* __restrict__ x, int B, int H, int W, int Cin,
                                                         int x_cs, int x_coff, const float* __restrict__ dy, int Ho,
                                                         int Wo, int Cout, int dy_cs, int dy_coff, int kh, int kw,
                                                         int s, int p, int d, float* __restrict__ dwp) {
  __shared__ float red[4][32 * 32];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int co0 = blockIdx.y * 32;
  const int cblocks = Cin / 32;
  const int tap = blockIdx.z / cblocks;
  const int ci0 = (blockIdx.z - tap * cblocks) * 32;
  const int ky = tap / kw, kx = tap - ky * kw;
  const long long P = (long long)B * Ho * Wo;
  const long long p0 = (long long)blockIdx.x * WG_PPB;
  const int kk = lane >> 4, r = lane & 15;
  f32x4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int g = wave; g < WG_PPB / 4; g += 4) {
    const long long pix = p0 + g * 4 + kk;
    float a0 = 0.f, a1 = 0.f, b0 = 0.f, b1 = 0.f;
    if (pix < P) {
      const float* dp = dy + pix * dy_cs + dy_coff + co0 + r;
      a0 = dp[0];
      a1 = dp[16];
      const int ox = (int)(pix % Wo);
      const long long rr = pix / Wo;
      const int oy = (int)(rr % Ho), b = (int)(rr / Ho);
      const int iy = oy * s - p + ky * d, ix = ox * s - p + kx * d;
      if (iy >= 0 && iy < H && ix >= 0 && ix < W) {
        const float* xp = x + (((long long)b * H + iy) * W + ix) * x_cs + x_coff + ci0 + r;
        b0 = xp[0];
        b1 = xp[16];
      }
    }
    acc[0][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b0, acc[0][0], 0, 0, 0);
    acc[0][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b1, acc[0][1], 0, 0, 0);
    acc[1][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b0, acc[1][0], 0, 0, 0);
    acc[1][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b1, acc[1][1], 0, 0, 0);
  }
  // C[row][col]: lane holds rows 4*(lane>>4)+q, col lane&15 of each 16x16 tile
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int row = i * 16 + kk * 4 + q, col = j * 16 + r;
        red[wave][row * 32 + col] = acc[i][j][q];
      }
  __syncthreads();
  const int KT = kh * kw * Cin;
  for (int e = threadIdx.x; e < 1024; e += 256) {
    const float v = red[0][e] + red[1][e] + red[2][e] + red[3][e];
    const int row = e >> 5, col = e & 31;
    atomicAdd(dwp + (size_t)(co0 + row) * KT + tap * Cin + ci0 + col, v);
  }
}

// ---------------------------------------------------------------------------
// weight layout transforms
// ---------------------------------------------------------------------------
__global__ void pack_weight_kernel(const float* __restrict__ w, float* __restrict__ o, int Co, int Ci, int kh, int kw,
                                   int mode) {
  const int taps = kh * kw;
  const long long n = (long long)Co * Ci * taps;
  GSTRIDE(i, n) {
    // i enumerates the SOURCE layout
    if (mode == 0 || mode == 1) {
      const int tap = (int)(i % taps);
      const long long r = i / taps;
      const int ci = (int)(r % Ci), co = (int)(r / Ci);
      if (mode == 0) {
        o[((size_t)co * taps + tap) * Ci + ci] = w[i];
      } else {
        const int ft = taps - 1 - tap;  // (kh-1-ky, kw-1-kx)
        o[((size_t)ci * taps + ft) * Co + co] = w[i];
      }
    } else {
      // ConvTranspose weight [Ci][Co][2][2] with Co, Ci as named in the call
      // (Ci = in_channels, Co = out_channels), q = a*2+b
      const int q = (int)(i % 4);
      const long long r = i / 4;
      const int co = (int)(r % Co), ci = (int)(r / Co);
      if (mode == 2) o[((size_t)q * Co + co) * Ci + ci] = w[i];
      else o[((size_t)ci * 4 + q) * Co + co] = w[i];
    }
  }
}

__global__ __launch_bounds__(256) void pack_batch_kernel(const UprPackJob* __restrict__ jobs) {
  const UprPackJob j = jobs[blockIdx.y];
  const int taps = j.kh * j.kw;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < j.n; i += gridDim.x * 256) {
    const float v = j.w[i];
    if (j.mode == 4) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        if (j.out32) j.out32[q * j.Co + i] = v;
        if (j.out16) ((half_t*)j.out16)[q * j.Co + i] = (half_t)v;
      }
      continue;
    }
    int dst;
    if (j.mode <= 1) {
      const int tap = i % taps, r = i / taps;
      const int ci = r % j.Ci, co = r / j.Ci;
      dst = j.mode == 0 ? (co * taps + tap) * j.Ci + ci : (ci * taps + (taps - 1 - tap)) * j.Co + co;
    } else {
      const int q = i % 4, r = i / 4;
      const int co = r % j.Co, ci = r / j.Co;
      dst = j.mode == 2 ? (q * j.Co + co) * j.Ci + ci : (ci * 4 + q) * j.Co + co;
    }
    if (j.out32) j.out32[dst] = v;
    if (j.out16) ((half_t*)j.out16)[dst] = (half_t)v;
  }
}

__global__ void unpack_grad_kernel(const float* __restrict__ gp, float* __restrict__ g, int Co, int Ci, int kh, int kw,
                                   int mode, int accum) {
  const int taps = kh * kw;
  const long long n = (long long)Co * Ci * taps;
  GSTRIDE(i, n) {
    float v;
    if (mode == 0) {
      const int tap = (int)(i % taps);
      const long long r = i / taps;
      const int ci = (int)(r % Ci), co = (int)(r / Ci);
      v = gp[((size_t)co * taps + tap) * Ci + ci];
    } else {
      const int q = (int)(i % 4);
      const long long r = i / 4;
      const int co = (int)(r % Co), ci = (int)(r / Co);
      v = gp[((size_t)ci * 4 + q) * Co + co];
    }
    g[i] = accum ? g[i] + v : v;
  }
}

// ---------------------------------------------------------------------------
// zero-upsampled output gradient: the operand of a stride-2 conv's input
// gradient, run as a stride-1 conv over it
// ---------------------------------------------------------------------------
__global__ void zero_upsample_kernel(const float* __restrict__ dy, int B, int Ho, int Wo, int C, int cs, int coff,
                                     float* __restrict__ z) {
  const long long n = (long long)B * 2 * Ho * 2 * Wo * C;
  GSTRIDE(i, n) {
    const int c = (int)(i % C);
    long long r = i / C;
    const int X = (int)(r % (2 * Wo)); r /= 2 * Wo;
    const int Y = (int)(r % (2 * Ho));
    const int b = (int)(r / (2 * Ho));
    float v = 0.f;
    if (!(X & 1) && !(Y & 1)) v = dy[(((long long)b * Ho + (Y >> 1)) * Wo + (X >> 1)) * cs + coff + c];
    z[i] = v;
  }
}

// fp16 form for the autocast stride-2 input gradient: dy (fp32) rounded to
// fp16 as the conv's cast would, zero-upsampled, 8 channels per thread
// from the gradient's compact fp16 copy (dy16 [B][Ho][Wo][C]): 16-byte copies
__global__ __launch_bounds__(256) void zero_upsample16h_kernel(const half_t* __restrict__ dy16, int B, int Ho, int Wo,
                                                               int C, half_t* __restrict__ z, long long n) {
  const int C8 = C / 8;
  GSTRIDE(i, n) {
    const int c = (int)(i % C8) * 8;
    long long r = i / C8;
    const int X = (int)(r % (2 * Wo)); r /= 2 * Wo;
    const int Y = (int)(r % (2 * Ho));
    const int b = (int)(r / (2 * Ho));
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (!(X & 1) && !(Y & 1)) v = *(const uint4*)(dy16 + (((long long)b * Ho + (Y >> 1)) * Wo + (X >> 1)) * C + c);
    *(uint4*)(z + i * 8) = v;
  }
}

__global__ __launch_bounds__(256) void zero_upsample16_kernel(const float* __restrict__ dy, int B, int Ho, int Wo,
                                                              int C, int cs, int coff, half_t* __restrict__ z) {
  typedef _Float16 h8 __attribute__((ext_vector_type(8)));
  const int C8 = C / 8;
  const long long n = (long long)B * 2 * Ho * 2 * Wo * C8;
  GSTRIDE(i, n) {
    const int c = (int)(i % C8) * 8;
    long long r = i / C8;
    const int X = (int)(r % (2 * Wo)); r /= 2 * Wo;
    const int Y = (int)(r % (2 * Ho));
    const int b = (int)(r / (2 * Ho));
    h8 v = h8{};
    if (!(X & 1) && !(Y & 1)) {
      const float* src = dy + (((long long)b * Ho + (Y >> 1)) * Wo + (X >> 1)) * cs + coff + c;
      const float4 lo = *(const float4*)src, hi = *(const float4*)(src + 4);
      v = h8{(half_t)lo.x, (half_t)lo.y, (half_t)lo.z, (half_t)lo.w, (half_t)hi.x, (half_t)hi.y, (half_t)hi.z,
             (half_t)hi.w};
    }
    *(h8*)(z + i * 8) = v;
  }
}

// ---- autocast (AMP) convs: fp16 operands, fp32 accumulate, fp32 activations ----
// x[m][coff + c] (fp32, pixel stride cs) -> dense fp16 [m][C], 8 channels per thread
__global__ __launch_bounds__(256) void cast_act_f16_kernel(const float* __restrict__ x, long long M, int C, int cs,
                                                           int coff, half_t* __restrict__ y) {
  const int C8 = C / 8;
  typedef _Float16 h8 __attribute__((ext_vector_type(8)));
  if (256 % C8 == 0) {  // fixed channels per thread, rows by addition (no 64-bit div per element)
    const int c = (threadIdx.x % C8) * 8, rpb = 256 / C8;
    for (long long m = (long long)blockIdx.x * rpb + threadIdx.x / C8; m < M; m += (long long)gridDim.x * rpb) {
      const float4* src = (const float4*)(x + m * cs + coff + c);
      const float4 a = src[0], b = src[1];
      *(h8*)(y + m * C + c) =
          h8{(half_t)a.x, (half_t)a.y, (half_t)a.z, (half_t)a.w, (half_t)b.x, (half_t)b.y, (half_t)b.z, (half_t)b.w};
    }
    return;
  }
  GSTRIDE(i, M * C8) {
    const long long m = i / C8;
    const int c = (int)(i - m * C8) * 8;
    const float4* src = (const float4*)(x + m * cs + coff + c);
    const float4 a = src[0], b = src[1];
    h8 o = {(half_t)a.x, (half_t)a.y, (half_t)a.z, (half_t)a.w, (half_t)b.x, (half_t)b.y, (half_t)b.z, (half_t)b.w};
    *(h8*)(y + m * C + c) = o;
  }
}
// dense fp16 [m][C] -> y[m][coff + c] (fp32) (+ res[m * res_cs + c], fp32; res may alias y)
__global__ __launch_bounds__(256) void cast_act_f32_kernel(const half_t* __restrict__ x, long long M, int C,
                                                           const float* res, int res_cs, float* y, int cs, int coff,
                                                           int xcs) {
  const int C4 = C / 4;
  GSTRIDE(i, M * C4) {
    const long long m = i / C4;
    const int c = (int)(i - m * C4) * 4;
    typedef _Float16 h4 __attribute__((ext_vector_type(4)));
    const h4 v = *(const h4*)(x + m * xcs + c);
    float4 o = make_float4((float)v[0], (float)v[1], (float)v[2], (float)v[3]);
    if (res) {
      const float4 r = *(const float4*)(res + m * res_cs + c);
      o.x += r.x; o.y += r.y; o.z += r.z; o.w += r.w;
    }
    *(float4*)(y + m * cs + coff + c) = o;
  }
}
__global__ __launch_bounds__(256) void cast_f16_kernel(const float* __restrict__ x, long long n, half_t* __restrict__ y) {
  GSTRIDE(i, n) y[i] = (half_t)x[i];
}

}  // namespace upr

using namespace upr;

// The argument checks of the four direct-conv entries (upr_t_conv_direct /
// _direct16 / _direct_dgrad / _direct_wgrad / _direct_wgrad_relu): a and b are
// the call's two activation views, p its weight (or weight-gradient) pointer
static int direct_conv_args(const UprView* a, const UprView* b, const void* p, int B, int H, int W, int Cin, int Cout,
                            int kh, int kw, int stride, int pad, int dil, int Ho, int Wo) {
  if (!a || !b || !a->data || !b->data || !p) return UPR_ERR_ARG;
  if (B <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0 || kh <= 0 || kw <= 0 || stride <= 0 || pad < 0 || dil <= 0)
    return UPR_ERR_ARG;
  const long long eh = (long long)H + 2ll * pad - (long long)dil * (kh - 1) - 1;
  const long long ew = (long long)W + 2ll * pad - (long long)dil * (kw - 1) - 1;
  if (eh < 0 || ew < 0 || Ho != eh / stride + 1 || Wo != ew / stride + 1) return UPR_ERR_SHAPE;
  return UPR_OK;
}

// The argument checks of upr_t_conv_wgrad / _wgrad16 / _wgrad_into beyond their
// pointers; every one of them comes before anything is queued
static int mfma_wgrad_args(int B, int H, int W, int Cin, int x_cs, int x_coff, int Ho, int Wo, int Cout, int dy_cs,
                           int dy_coff, int kh, int kw, int stride, int pad, int dil) {
  if (B <= 0 || Cin % 32 || Cout % 32 || Cin <= 0 || Cout <= 0) return UPR_ERR_ARG;
  if (H <= 0 || W <= 0 || Ho <= 0 || Wo <= 0 || kh <= 0 || kw <= 0 || stride <= 0 || pad < 0 || dil <= 0)
    return UPR_ERR_ARG;
  if (x_coff < 0 || dy_coff < 0 || (long long)x_cs < (long long)x_coff + Cin ||
      (long long)dy_cs < (long long)dy_coff + Cout)
    return UPR_ERR_ARG;
  const long long eh = (long long)H + 2ll * pad - (long long)dil * (kh - 1) - 1;
  const long long ew = (long long)W + 2ll * pad - (long long)dil * (kw - 1) - 1;
  if (eh < 0 || ew < 0 || Ho != eh / stride + 1 || Wo != ew / stride + 1) return UPR_ERR_SHAPE;
  return UPR_OK;
}

extern "C" {

int upr_t_conv_direct(const UprView* x, int B, int H, int W, int Cin, const float* w, const float* bias, int Cout,
                      int kh, int kw, int stride, int pad, int dil, const UprView* y, int Ho, int Wo, int relu,
                      int accumulate, void* stream) {
  if (const int bad = direct_conv_args(x, y, w, B, H, W, Cin, Cout, kh, kw, stride, pad, dil, Ho, Wo)) return bad;
  {
    const int rc = small_conv_fwd(x, B, H, W, Cin, w, bias, Cout, kh, kw, stride, pad, dil, y, Ho, Wo, relu,
                                  accumulate, ST(stream));
    if (rc != kErrUnsupported) return rc;
  }
  const long long n = (long long)B * Ho * Wo * Cout;
  if (Cin == 3 && kh == 3 && kw == 3 && stride == 1 && dil == 1) {
    hipLaunchKernelGGL(conv_direct_c3k3_kernel, dim3(grid_for(n)), dim3(256), 0, ST(stream), mkv(x), B, H, W, w, bias,
                       Cout, pad, mkv(y), Ho, Wo, relu, accumulate);
    LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(conv_direct_kernel, dim3(grid_for(n)), dim3(256), 0, ST(stream), mkv(x), B, H, W, Cin, w, bias,
                     Cout, kh, kw, stride, pad, dil, mkv(y), Ho, Wo, relu, accumulate);
  LAUNCH_CHECK();
}

int upr_t_conv_dgrad_c3_16(const void* dy16, int B, int H, int W, const float* w, int Cout, const UprView* dx,
                           int accumulate, void* stream) {
  if (!dy16 || !w || !dx || !dx->data || B <= 0 || H <= 0 || W <= 0) return UPR_ERR_ARG;
  const int rc = small_conv_dgrad_c3_16(dy16, B, H, W, w, Cout, dx, accumulate, ST(stream));
  return rc == kErrUnsupported ? UPR_ERR_UNSUPPORTED : rc;
}

int upr_t_conv_direct16(const UprView* x, int B, int H, int W, int Cin, const float* w, const float* bias, int Cout,
                        int kh, int kw, int stride, int pad, int dil, const UprView* y, int Ho, int Wo, int relu,
                        int accumulate, void* y16, int skip32, void* stream) {
  if (!y16 || (skip32 && accumulate)) return UPR_ERR_ARG;
  if (const int bad = direct_conv_args(x, y, w, B, H, W, Cin, Cout, kh, kw, stride, pad, dil, Ho, Wo)) return bad;
  const int rc = small_conv_fwd(x, B, H, W, Cin, w, bias, Cout, kh, kw, stride, pad, dil, y, Ho, Wo, relu, accumulate,
                                ST(stream), y16, skip32);
  return rc == kErrUnsupported ? UPR_ERR_UNSUPPORTED : rc;
}

int upr_t_conv_direct_dgrad(const UprView* dy, int Ho, int Wo, const float* w, int B, int H, int W, int Cin, int Cout,
                            int kh, int kw, int stride, int pad, int dil, const UprView* dx, int accumulate,
                            void* stream) {
  if (const int bad = direct_conv_args(dy, dx, w, B, H, W, Cin, Cout, kh, kw, stride, pad, dil, Ho, Wo)) return bad;
  {
    const int rc = small_conv_dgrad(dy, Ho, Wo, w, B, H, W, Cin, Cout, kh, kw, stride, pad, dil, dx, accumulate,
                                    ST(stream));
    if (rc != kErrUnsupported) return rc;
  }
  const long long n = (long long)B * H * W * Cin;
  hipLaunchKernelGGL(conv_direct_dgrad_kernel, dim3(grid_for(n)), dim3(256), 0, ST(stream), mkv(dy), Ho, Wo, w, B, H,
                     W, Cin, Cout, kh, kw, stride, pad, dil, mkv(dx), accumulate);
  LAUNCH_CHECK();
}

int upr_t_conv_stem_wgrad_relu16(const UprView* x, const float* dy, const void* y16, int B, int H, int W, float* dw,
                                 float* dbias, void* stream) {
  if (!x || !dy || !y16 || !dw || !dbias || B <= 0 || H <= 0 || W <= 0) return UPR_ERR_ARG;
  const int rc = small_stem_wgrad_relu16(x, dy, y16, B, H, W, dw, dbias, ST(stream));
  return rc == kErrUnsupported ? UPR_ERR_UNSUPPORTED : rc;
}

int upr_t_conv_direct_wgrad_relu(const UprView* x, const UprView* dy, const UprView* y, int B, int H, int W, int Cin,
                                 int Ho, int Wo, int Cout, int kh, int kw, int stride, int pad, int dil, float* dw,
                                 float* dbias, void* stream) {
  if (!y || !y->data) return UPR_ERR_ARG;
  if (const int bad = direct_conv_args(x, dy, dw, B, H, W, Cin, Cout, kh, kw, stride, pad, dil, Ho, Wo)) return bad;
  const int rc = small_conv_wgrad(x, dy, B, H, W, Cin, Ho, Wo, Cout, kh, kw, stride, pad, dil, dw, dbias, ST(stream),
                                  y);
  return rc == kErrUnsupported ? UPR_ERR_UNSUPPORTED : rc;
}

int upr_t_conv_direct_wgrad(const UprView* x, const UprView* dy, int B, int H, int W, int Cin, int Ho, int Wo,
                            int Cout, int kh, int kw, int stride, int pad, int dil, float* dw, float* dbias,
                            void* stream) {
  if (const int bad = direct_conv_args(x, dy, dw, B, H, W, Cin, Cout, kh, kw, stride, pad, dil, Ho, Wo)) return bad;
  {
    const int rc = small_conv_wgrad(x, dy, B, H, W, Cin, Ho, Wo, Cout, kh, kw, stride, pad, dil, dw, dbias, ST(stream));
    if (rc != kErrUnsupported) return rc;
  }
  const int KC = kh * kw * Cin;
  const int nE = Cout * KC + (dbias ? Cout : 0);
  if (nE > 16 * 256) return UPR_ERR_UNSUPPORTED;
  int CH = 12288 / (Cout + KC);
  if (CH > 64) CH = 64;
  if (CH < 1) return UPR_ERR_UNSUPPORTED;
  const long long P = (long long)B * Ho * Wo;
  const int grid = grid_for(P, CH, 1024);
  const size_t lds = sizeof(float) * CH * (Cout + KC);
  float* part = (float*)scratch(kSlotPart, sizeof(float) * (size_t)grid * Cout * (KC + 1), ST(stream));
  if (!part) return (int)hipErrorOutOfMemory;
  hipLaunchKernelGGL(conv_direct_wgrad_kernel, dim3(grid), dim3(256), lds, ST(stream), mkv(x), mkv(dy), B, H, W, Cin,
                     Ho, Wo, Cout, kh, kw, stride, pad, dil, CH, dbias != nullptr, part);
  return small_wgrad_finish(part, grid, Cout, KC, dw, dbias, ST(stream));
}

int upr_t_conv_mfma(const float* x, int B, int H, int W, int Cin, int x_cs, int x_coff, const float* wp,
                    const float* bias, int N, int kh, int kw, int stride, int pad, int dil, const float* res,
                    int res_cs, int relu, float* y, int y_cs, int y_coff, int store, void* stream) {
  if (!x || !wp || !y || B <= 0 || Cin % 32 || N % 32 || Cin <= 0 || N <= 0) return UPR_ERR_ARG;
  if (kh <= 0 || kw <= 0 || stride <= 0 || dil <= 0 || pad < 0) return UPR_ERR_ARG;
  if (x_cs % 4 || x_coff % 4 || y_cs % 4 || y_coff % 4 || (res && res_cs % 4)) return UPR_ERR_ARG;
  if (store == UPR_T_STORE_CONVT2X2 && ((N / 4) % 32)) return UPR_ERR_SHAPE;
  const int Ho = (H + 2 * pad - dil * (kh - 1) - 1) / stride + 1;
  const int Wo = (W + 2 * pad - dil * (kw - 1) - 1) / stride + 1;
  if (Ho <= 0 || Wo <= 0) return UPR_ERR_SHAPE;
  ConvOp c;
  memset(&c, 0, sizeof(c));
  c.nseg = 1;
  ConvSeg& s = c.seg[0];
  s.src = x; s.C = Cin; s.cs = x_cs; s.coff = x_coff; s.Hin = H; s.Win = W;
  s.kh = kh; s.kw = kw; s.stride = stride; s.pad = pad; s.dil = dil; s.pre = kPreNone; s.kbase = 0;
  c.B = B; c.Ho = Ho; c.Wo = Wo; c.N = N; c.Kpad = kh * kw * Cin;
  c.W = wp; c.bias = bias; c.res1 = res; c.res1_cs = res_cs; c.relu = relu;
  c.out = y; c.out_cs = y_cs; c.out_coff = y_coff; c.store = store == UPR_T_STORE_CONVT2X2 ? kStoreConvT2x2 : kStoreNHWC;
  return launch_conv(c, kF32, ST(stream));
}

int upr_t_cast_f16(const float* x, void* y, size_t n, void* stream) {
  if (!x || !y) return UPR_ERR_ARG;
  hipLaunchKernelGGL(cast_f16_kernel, dim3(grid_for((long long)n)), dim3(256), 0, ST(stream), x, (long long)n,
                     (half_t*)y);
  LAUNCH_CHECK();
}

int upr_t_conv_mfma16(const float* x, int B, int H, int W, int Cin, int x_cs, int x_coff, const void* wp16,
                      const float* bias, int N, int kh, int kw, int stride, int pad, int dil, const float* res,
                      int res_cs, int relu, float* y, int y_cs, int y_coff, int store, void* x16, int x16_ready,
                      void* y16, int y16_cs, void* stream) {
  if (!x16 || !wp16 || !y || !y16 || B <= 0 || Cin % 32 || N % 32 || Cin <= 0 || N <= 0) return UPR_ERR_ARG;
  if (!x16_ready && !x) return UPR_ERR_ARG;
  const bool want16 = (store & UPR_T_STORE_KEEP16) != 0;  // y16 must end up holding (half)y
  const bool only16 = want16 && (store & UPR_T_STORE_ONLY16) != 0;  // y itself not needed (written only on the fallback path)
  // the 1x1 stride-2 conv's input gradient (y = 2H x 2W, accumulated into at the even pixels)
  const bool s2 = (store & UPR_T_STORE_S2_1X1) != 0;
  // the 3x3 stride-2 pad-1 conv's input gradient from dy itself (x16 = dy over H x W, wp16 the
  // flipped filter, y = 2H x 2W); UPR_ERR_UNSUPPORTED when the kernel does not take the shape
  const bool s2dg = (store & UPR_T_STORE_S2_3X3_DGRAD) != 0;
  // the ready x16 keeps x's channel stride (a slice of a concat's fp16 copy)
  const bool x16_strided = (store & UPR_T_STORE_X16_STRIDED) != 0;
  store &= UPR_T_STORE_CONVT2X2;
  if (x16_strided && (!x16_ready || x_cs % 8 || x_cs < Cin || (uintptr_t)x16 % 16)) return UPR_ERR_ARG;
  if (s2 && (kh != 1 || kw != 1 || stride != 1 || pad != 0 || dil != 1 || store != 0 || !res || relu)) return UPR_ERR_ARG;
  if (s2dg && (s2 || kh != 3 || kw != 3 || stride != 1 || dil != 1 || store != 0 || relu || bias)) return UPR_ERR_ARG;
  const int ycs16 = y16_cs > 0 ? y16_cs : (store == UPR_T_STORE_CONVT2X2 ? N / 4 : N);  // y16's channel stride
  if (ycs16 % 8 || ((uintptr_t)y16 & 15)) return UPR_ERR_ARG;
  if (kh <= 0 || kw <= 0 || stride <= 0 || dil <= 0 || pad < 0) return UPR_ERR_ARG;
  if (x_cs % 4 || x_coff % 4 || y_cs % 4 || y_coff % 4 || (res && res_cs % 4)) return UPR_ERR_ARG;
  if (res && relu) return UPR_ERR_ARG;  // the residual is added in fp32 after the fp16 GEMM
  if (store == UPR_T_STORE_CONVT2X2 && ((N / 4) % 32)) return UPR_ERR_SHAPE;
  const int Ho = (H + 2 * pad - dil * (kh - 1) - 1) / stride + 1;
  const int Wo = (W + 2 * pad - dil * (kw - 1) - 1) / stride + 1;
  if (Ho <= 0 || Wo <= 0) return UPR_ERR_SHAPE;
  hipStream_t st = ST(stream);
  const long long Mi = (long long)B * H * W;
  ConvOp c;
  memset(&c, 0, sizeof(c));
  c.nseg = 1;
  ConvSeg& s = c.seg[0];
  s.src = x16; s.C = Cin; s.cs = x16_strided ? x_cs : Cin; s.coff = 0; s.Hin = H; s.Win = W;
  s.kh = kh; s.kw = kw; s.stride = stride; s.pad = pad; s.dil = dil; s.pre = kPreNone; s.kbase = 0;
  c.B = B; c.Ho = Ho; c.Wo = Wo; c.N = N; c.Kpad = kh * kw * Cin;
  c.W = wp16; c.bias = bias; c.relu = relu;
  c.store = store == UPR_T_STORE_CONVT2X2 ? kStoreConvT2x2 : kStoreNHWC;
  // the fp32 output (+ fp32 residual / accumulated gradient) straight from the conv epilogue
  ConvOp c32 = c;
  c32.out32 = y; c32.out32_cs = y_cs; c32.out32_coff = y_coff;
  c32.res32 = res; c32.res32_cs = res_cs;
  if (want16) { c32.out32_h16 = y16; c32.out32_h16_cs = ycs16; }
  c32.skip32 = only16 ? 1 : 0;
  c32.out_s2 = s2 ? 1 : 0;
  ConvOp cdg = c;
  if (s2dg) {
    cdg.Ho = 2 * H; cdg.Wo = 2 * W;
    cdg.out32 = y; cdg.out32_cs = y_cs; cdg.out32_coff = y_coff;
    cdg.res32 = res; cdg.res32_cs = res_cs;
    if (want16) { cdg.out32_h16 = y16; cdg.out32_h16_cs = ycs16; }
    cdg.skip32 = only16 ? 1 : 0;
  }
  // the forms only one kernel implements decline BEFORE the operand cast is queued
  if (s2dg && launch_conv_s2dg(cdg, st, true) == kErrUnsupported) return UPR_ERR_UNSUPPORTED;
  if (s2 && launch_conv_pw(c32, st, true) == kErrUnsupported) return UPR_ERR_UNSUPPORTED;
  if (!x16_ready) {
    if ((uintptr_t)x % 16 || x_cs % 8 || x_coff % 8) return UPR_ERR_ARG;
    hipLaunchKernelGGL(cast_act_f16_kernel, dim3(grid_for(Mi * (Cin / 8))), dim3(256), 0, st, x, Mi, Cin, x_cs, x_coff,
                       (half_t*)x16);
    UPR_CHECK_HIP(hipGetLastError());
  }
  if (s2dg) {
    const int rc = launch_conv_s2dg(cdg, st);
    if (rc == kErrUnsupported) return UPR_ERR_UNSUPPORTED;
    if (rc != 0) return rc;
    LAUNCH_CHECK();
  }
  {
    const int rc = launch_conv_out32(c32, st);
    if (rc != kErrUnsupported) {
      if (rc != 0) return rc;
      LAUNCH_CHECK();
    }
    if (s2) return UPR_ERR_UNSUPPORTED;  // no other kernel scatters at stride 2
  }
  c.out = y16; c.out_cs = ycs16; c.out_coff = 0;
  const int rc = launch_conv(c, kF16, st);
  if (rc != 0) return rc;
  const long long Mo = store == UPR_T_STORE_CONVT2X2 ? (long long)B * 4 * Ho * Wo : (long long)B * Ho * Wo;
  const int Co = store == UPR_T_STORE_CONVT2X2 ? N / 4 : N;
  hipLaunchKernelGGL(cast_act_f32_kernel, dim3(grid_for(Mo * (Co / 4))), dim3(256), 0, st, (const half_t*)y16, Mo, Co,
                     res, res_cs, y, y_cs, y_coff, ycs16);
  LAUNCH_CHECK();
}

int upr_t_conv_mfma16_relu_bwd(const void* x16, int B, int H, int W, int Cin, const void* wp16, int N, int kh, int kw,
                               int pad, int dil, float* y, int y_cs, int y_coff, void* y16, int y16_cs,
                               const void* mask16, int mask16_cs, int skip32, void* stream) {
  return upr_t_conv_mfma16_relu_bwd_cs(x16, Cin, B, H, W, Cin, wp16, N, kh, kw, pad, dil, y, y_cs, y_coff, y16, y16_cs,
                                       mask16, mask16_cs, skip32, stream);
}

int upr_t_conv_mfma16_relu_bwd_cs(const void* x16, int x16_cs, int B, int H, int W, int Cin, const void* wp16, int N,
                                  int kh, int kw, int pad, int dil, float* y, int y_cs, int y_coff, void* y16,
                                  int y16_cs, const void* mask16, int mask16_cs, int skip32, void* stream) {
  if (!x16 || !wp16 || !y || !y16 || !mask16 || B <= 0 || Cin % 32 || N % 32 || Cin <= 0 || N <= 0) return UPR_ERR_ARG;
  if (kh <= 0 || kw <= 0 || dil <= 0 || pad < 0 || x16_cs < Cin) return UPR_ERR_ARG;
  if (((uintptr_t)x16 | (uintptr_t)y16 | (uintptr_t)mask16) % 16 || y16_cs % 8 || mask16_cs % 8 || y_cs % 4 ||
      y_coff % 4 || (uintptr_t)y % 16 || x16_cs % 8)
    return UPR_ERR_UNSUPPORTED;
  const int Ho = H + 2 * pad - dil * (kh - 1), Wo = W + 2 * pad - dil * (kw - 1);
  if (Ho <= 0 || Wo <= 0) return UPR_ERR_SHAPE;
  ConvOp c;
  memset(&c, 0, sizeof(c));
  c.nseg = 1;
  ConvSeg& sg = c.seg[0];
  sg.src = x16; sg.C = Cin; sg.cs = x16_cs; sg.coff = 0; sg.Hin = H; sg.Win = W;
  sg.kh = kh; sg.kw = kw; sg.stride = 1; sg.pad = pad; sg.dil = dil; sg.pre = kPreNone; sg.kbase = 0;
  c.B = B; c.Ho = Ho; c.Wo = Wo; c.N = N; c.Kpad = kh * kw * Cin;
  c.W = wp16; c.bias = nullptr; c.relu = 0;
  c.store = kStoreNHWC;
  c.out32 = y; c.out32_cs = y_cs; c.out32_coff = y_coff;
  c.out32_h16 = y16; c.out32_h16_cs = y16_cs;
  c.mask16 = mask16; c.mask16_cs = mask16_cs; c.skip32 = skip32 ? 1 : 0;
  const int rc = launch_conv_out32(c, ST(stream));
  if (rc == kErrUnsupported) return UPR_ERR_UNSUPPORTED;
  if (rc != 0) return rc;
  LAUNCH_CHECK();
}

int upr_t_conv_wgrad(const float* x, int B, int H, int W, int Cin, int x_cs, int x_coff, const float* dy, int Ho,
                     int Wo, int Cout, int dy_cs, int dy_coff, int kh, int kw, int stride, int pad, int dil,
                     float* dwp, void* stream) {
  wgrad_ran_set(UPR_WGRAD_NONE);
  if (!x || !dy || !dwp) return UPR_ERR_ARG;
  if (const int bad = mfma_wgrad_args(B, H, W, Cin, x_cs, x_coff, Ho, Wo, Cout, dy_cs, dy_coff, kh, kw, stride, pad, dil))
    return bad;
  {
    const int rc = wgrad_gemm(x, B, H, W, Cin, x_cs, x_coff, dy, Ho, Wo, Cout, dy_cs, dy_coff, kh, kw, stride, pad, dil,
                              dwp, ST(stream));
    if (rc != kErrUnsupported) return rc;
  }
  const long long P = (long long)B * Ho * Wo;
  const long long chunks = (P + WG_PPB - 1) / WG_PPB;
  if (chunks > 0x7fffffff) return UPR_ERR_SHAPE;
  dim3 grid((unsigned)chunks, Cout / 32, kh * kw * (Cin / 32));
  hipLaunchKernelGGL(conv_wgrad_kernel, grid, dim3(256), 0, ST(stream), x, B, H, W, Cin, x_cs, x_coff, dy, Ho, Wo,
                     Cout, dy_cs, dy_coff, kh, kw, stride, pad, dil, dwp);
  wgrad_ran_set(UPR_WGRAD_TAP32, 32, 32, 0, (int)chunks);
  LAUNCH_CHECK();
}

int upr_t_conv_wgrad16(const float* x, const void* x16, int B, int H, int W, int Cin, int x_cs, int x_coff,
                       const float* dy, int Ho, int Wo, int Cout, int dy_cs, int dy_coff, int kh, int kw, int stride,
                       int pad, int dil, float* dwp, void* stream) {
  wgrad_ran_set(UPR_WGRAD_NONE);
  if ((!x && !x16) || !dy || !dwp) return UPR_ERR_ARG;
  if (const int bad = mfma_wgrad_args(B, H, W, Cin, x_cs, x_coff, Ho, Wo, Cout, dy_cs, dy_coff, kh, kw, stride, pad, dil))
    return bad;
  hipStream_t st = ST(stream);
  const bool fits = Wo % 64 == 0 && dy_cs % 4 == 0 && dy_coff % 4 == 0 && (uintptr_t)dy % 16 == 0 &&
                    (uintptr_t)dwp % 16 == 0 && (x16 || (x && x_cs % 8 == 0 && x_coff % 8 == 0 && (uintptr_t)x % 16 == 0));
  if (fits) {
    void* tmp = nullptr;
    const void* src = x16;
    if (!src) {
      const long long Mi = (long long)B * H * W;
      tmp = scratch(kSlotCast, (size_t)Mi * Cin * sizeof(half_t), st);
      if (!tmp) return (int)hipErrorOutOfMemory;
      hipLaunchKernelGGL(cast_act_f16_kernel, dim3(grid_for(Mi * (Cin / 8))), dim3(256), 0, st, x, Mi, Cin, x_cs, x_coff,
                         (half_t*)tmp);
      src = tmp;
    }
    const int rc = wgrad16_gemm(src, B, H, W, Cin, dy, Ho, Wo, Cout, dy_cs, dy_coff, kh, kw, stride, pad, dil, dwp, st);
    if (rc != kErrUnsupported) return rc;
  }
  if (!x) return UPR_ERR_ARG;
  return upr_t_conv_wgrad(x, B, H, W, Cin, x_cs, x_coff, dy, Ho, Wo, Cout, dy_cs, dy_coff, kh, kw, stride, pad, dil, dwp,
                          stream);
}

int upr_t_conv_wgrad_into(const float* x, const void* x16, int B, int H, int W, int Cin, int x_cs, int x_coff,
                          const float* dy, const void* dy16, int Ho, int Wo, int Cout, int dy_cs, int dy_coff, int kh,
                          int kw, int stride, int pad, int dil, float* dw, void* stream) {
  wgrad_ran_set(UPR_WGRAD_NONE);
  if ((!x && !x16) || !dy || !dw) return UPR_ERR_ARG;
  if (const int bad = mfma_wgrad_args(B, H, W, Cin, x_cs, x_coff, Ho, Wo, Cout, dy_cs, dy_coff, kh, kw, stride, pad, dil))
    return bad;
  hipStream_t st = ST(stream);
  if (x16) {
    const int rc = wgrad16_gemm(x16, B, H, W, Cin, dy, Ho, Wo, Cout, dy_cs, dy_coff, kh, kw, stride, pad, dil, dw, st,
                                Cin, dy16);
    if (rc != kErrUnsupported) return rc;
  }
  if (!x) return UPR_ERR_ARG;
  {
    const int rc = wgrad_gemm(x, B, H, W, Cin, x_cs, x_coff, dy, Ho, Wo, Cout, dy_cs, dy_coff, kh, kw, stride, pad, dil,
                              dw, st, Cin);
    if (rc != kErrUnsupported) return rc;
  }
  // any other shape: the packed form into scratch, then added in PyTorch's layout
  const size_t n = (size_t)Cout * Cin * kh * kw;
  float* tmp = nullptr;
  tmp = (float*)scratch(kSlotTmp, n * sizeof(float), st);
  if (!tmp) return (int)hipErrorOutOfMemory;
  UPR_CHECK_HIP(hipMemsetAsync(tmp, 0, n * sizeof(float), st));
  int rc = x16 ? upr_t_conv_wgrad16(x, x16, B, H, W, Cin, x_cs, x_coff, dy, Ho, Wo, Cout, dy_cs, dy_coff, kh, kw, stride,
                                    pad, dil, tmp, stream)
               : upr_t_conv_wgrad(x, B, H, W, Cin, x_cs, x_coff, dy, Ho, Wo, Cout, dy_cs, dy_coff, kh, kw, stride, pad,
                                  dil, tmp, stream);
  if (rc == UPR_OK) rc = upr_t_unpack_grad(tmp, dw, Cout, Cin, kh, kw, 0, 1, stream);
  return rc;
}

int upr_t_conv_wgrad_ran(UprWgradRan* out) {
  if (!out) return UPR_ERR_ARG;
  *out = wgrad_ran();
  return UPR_OK;
}

int upr_t_pack_weight(const float* w, float* out, int Co, int Ci, int kh, int kw, int mode, void* stream) {
  if (!w || !out || Co <= 0 || Ci <= 0 || mode < 0 || mode > 3) return UPR_ERR_ARG;
  if (mode >= 2 && (kh != 2 || kw != 2)) return UPR_ERR_SHAPE;
  const long long n = (long long)Co * Ci * kh * kw;
  hipLaunchKernelGGL(pack_weight_kernel, dim3(grid_for(n)), dim3(256), 0, ST(stream), w, out, Co, Ci, kh, kw, mode);
  LAUNCH_CHECK();
}

int upr_t_pack_weights(const UprPackJob* jobs, int njobs, int max_n, void* stream) {
  if (!jobs || njobs < 0 || max_n < 0 || njobs > 65535) return UPR_ERR_ARG;
  if (njobs == 0 || max_n == 0) return UPR_OK;
  const int gx = (max_n + 255) / 256 < 64 ? (max_n + 255) / 256 : 64;
  hipLaunchKernelGGL(pack_batch_kernel, dim3(gx, njobs), dim3(256), 0, ST(stream), jobs);
  LAUNCH_CHECK();
}

int upr_t_unpack_grad(const float* gp, float* g, int Co, int Ci, int kh, int kw, int mode, int accumulate,
                      void* stream) {
  if (!gp || !g || (mode != 0 && mode != 3)) return UPR_ERR_ARG;
  const long long n = (long long)Co * Ci * kh * kw;
  hipLaunchKernelGGL(unpack_grad_kernel, dim3(grid_for(n)), dim3(256), 0, ST(stream), gp, g, Co, Ci, kh, kw, mode,
                     accumulate);
  LAUNCH_CHECK();
}

int upr_t_zero_upsample(const float* dy, int B, int Ho, int Wo, int C, int dy_cs, int dy_coff, float* z,
                        void* stream) {
  if (!dy || !z) return UPR_ERR_ARG;
  const long long n = (long long)B * 4 * Ho * Wo * C;
  hipLaunchKernelGGL(zero_upsample_kernel, dim3(grid_for(n)), dim3(256), 0, ST(stream), dy, B, Ho, Wo, C, dy_cs,
                     dy_coff, z);
  LAUNCH_CHECK();
}

int upr_t_zero_upsample16(const float* dy, int B, int Ho, int Wo, int C, int dy_cs, int dy_coff, void* z16,
                          void* stream) {
  if (!dy || !z16 || C % 8 || dy_cs % 4 || dy_coff % 4 || ((uintptr_t)dy & 15) || ((uintptr_t)z16 & 15))
    return UPR_ERR_ARG;
  const long long n = (long long)B * 4 * Ho * Wo * (C / 8);
  hipLaunchKernelGGL(zero_upsample16_kernel, dim3(grid_for(n)), dim3(256), 0, ST(stream), dy, B, Ho, Wo, C, dy_cs,
                     dy_coff, (half_t*)z16);
  LAUNCH_CHECK();
}

int upr_t_zero_upsample16h(const void* dy16, int B, int Ho, int Wo, int C, void* z16, void* stream) {
  if (!dy16 || !z16 || C % 8 || ((uintptr_t)dy16 & 15) || ((uintptr_t)z16 & 15)) return UPR_ERR_ARG;
  const long long n = (long long)B * 4 * Ho * Wo * (C / 8);
  hipLaunchKernelGGL(zero_upsample16h_kernel, dim3(grid_for(n)), dim3(256), 0, ST(stream), (const half_t*)dy16, B, Ho,
                     Wo, C, (half_t*)z16, n);
  LAUNCH_CHECK();
}

}  // extern "C"
