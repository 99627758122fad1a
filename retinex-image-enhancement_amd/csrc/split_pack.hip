// The split forms of the fp32 forward: the two host-side weight packers, the
// fp32 <-> split-fp16 tensor kernels, and the reader of the switches.
#include <algorithm>
#include <cmath>
#include <cstdlib>

#include "split_pack.h"

namespace upr {

// ---------------------------------------------------------------------------
// Split-fp16 form of an fp32 GEMM (the fp16 wide-tile kernel computing an fp32
// conv, ConvOp::split_out).  Activations: v = hi + lo * 2^-11, both fp16.
// Weights, per output channel n: a power of two s_n puts max|w| in [2^14,
// 2^15) (exact), W_hi = fp16(w s), W_lo = fp16(w s - W_hi).  Then
//   x w s ~= hi W_hi + lo (W_hi 2^-11) + hi W_lo        (fp32 accumulate)
// and the dropped lo W_lo term is ~2^-22 relative.  Each logical segment (src,
// C, taps) becomes two K-segments over the same [hi | lo] source of pixel
// stride 2C: A reads all 2C channels against [W_hi | W_hi 2^-11] per tap, B
// reads the C hi channels against W_lo.  scale[n] = 1 / s_n (the epilogue
// applies it before the bias).  Scaling the weights up keeps W_lo and the lo
// products clear of the fp16 subnormal range; storing lo scaled by 2^11 does
// the same for the activations.
// ---------------------------------------------------------------------------
bool pack_split(int N, const std::vector<SegWeights>& segs, SplitPack& out) {
  if (segs.empty() || segs.size() > 2) return false;
  out = SplitPack();
  out.N = N;
  int K = 0;
  for (const auto& s : segs) {
    const SegSpec& sp = s.spec;
    if (sp.coff != 0 || sp.cs != sp.C || sp.C % 64 || sp.pre != kPreNone) return false;
    const int taps = sp.kh * sp.kw;
    SegSpec a = sp, b = sp;
    a.C = 2 * sp.C; a.cs = 2 * sp.C; a.kbase = K;
    K += taps * 2 * sp.C;
    b.C = sp.C; b.cs = 2 * sp.C; b.kbase = K;
    K += taps * sp.C;
    out.segs.push_back(a);
    out.segs.push_back(b);
  }
  out.Kpad = (int)align_up(K, 32);
  out.W.assign((size_t)N * out.Kpad, (_Float16)0.f);
  out.scale.assign(N, 1.f);
  for (int n = 0; n < N; ++n) {
    double mx = 0.0;
    for (const auto& s : segs) {
      const size_t per = (size_t)s.spec.C * s.spec.kh * s.spec.kw;
      for (size_t i = 0; i < per; ++i) mx = std::max(mx, std::fabs(s.w[n * per + i]));
    }
    int e = 15;  // mx = f 2^e, f in [0.5, 1): mx 2^(15 - e) is in [2^14, 2^15)
    if (mx > 0.0 && std::isfinite(mx)) (void)std::frexp(mx, &e);
    const int sh = std::min(std::max(15 - e, -100), 100);
    const double sc = std::ldexp(1.0, sh);
    out.scale[n] = (float)std::ldexp(1.0, -sh);
    for (size_t si = 0; si < segs.size(); ++si) {
      const SegSpec& sp = segs[si].spec;
      const int C = sp.C, kh = sp.kh, kw = sp.kw;
      _Float16* rowA = out.W.data() + (size_t)n * out.Kpad + out.segs[2 * si].kbase;
      _Float16* rowB = out.W.data() + (size_t)n * out.Kpad + out.segs[2 * si + 1].kbase;
      for (int c = 0; c < C; ++c)
        for (int r = 0; r < kh; ++r)
          for (int q = 0; q < kw; ++q) {
            const double w = segs[si].w[(((size_t)n * C + c) * kh + r) * kw + q] * sc;
            const _Float16 hi = (_Float16)w;
            const int t = r * kw + q;
            rowA[t * 2 * C + c] = hi;
            rowA[t * 2 * C + C + c] = (_Float16)((double)hi * (1.0 / 2048.0));
            rowB[t * C + c] = (_Float16)(w - (double)hi);
          }
    }
  }
  return true;
}

// ---------------------------------------------------------------------------
// Weights split once (ConvOp::mma16 == kMma16WSplit, conv_wide32.hip): the
// fp32 tensors stay as they are and the kernel splits its activation
// fragments in registers; only the weights are prepared here.  w: the packed
// fp32 [N][K] rows of pack_gemm (K-segments of C % 32 == 0 channels, so every
// 32 consecutive k are 32 channels of one tap).  Per row n: s_n from
// split_row_shift over the row (the rule of pack_split and of the ring's
// prologue), W_hi = fp16(w s_n), W_lo = fp16(w s_n - W_hi), stored per 32-deep
// K step as [W_hi(32) | W_lo(32)] in k-slot order (wsplit_kslot); scale[n] =
// 1 / s_n.  A row takes 4 K bytes, as the fp32 row does.
// ---------------------------------------------------------------------------
bool pack_split_w(int N, int K, const float* w, SplitWPack& out) {
  if (!w || N <= 0 || N % 64 || K <= 0 || K % 32) return false;
  out.W.assign((size_t)N * K * 2, (_Float16)0.f);
  out.scale.assign(N, 1.f);
  for (int n = 0; n < N; ++n) {
    const float* row = w + (size_t)n * K;
    float mx = 0.f;
    for (int k = 0; k < K; ++k) mx = std::max(mx, std::fabs(row[k]));
    const int sh = split_row_shift(mx);
    const float s = std::ldexp(1.f, sh);
    out.scale[n] = std::ldexp(1.f, -sh);
    _Float16* dst = out.W.data() + (size_t)n * K * 2;
    for (int k = 0; k < K; ++k) {
      const float ws = row[k] * s;
      const _Float16 hi = (_Float16)ws;
      _Float16* step = dst + (size_t)(k / 32) * 64;
      step[wsplit_kslot(k % 32)] = hi;
      step[32 + wsplit_kslot(k % 32)] = (_Float16)(ws - (float)hi);
    }
  }
  return true;
}

size_t split_w_bytes(int Cout, int K, size_t* scale_off) {
  const size_t wbytes = align_up((size_t)Cout * K * 4, 256);
  if (scale_off) *scale_off = wbytes;
  return wbytes + (size_t)Cout * 4;
}

// fp32 NHWC <-> split fp16 ([hi(C) | lo(C)] per pixel, ConvOp::split_out):
// one thread per 8 channels of a pixel, 16-byte accesses
__global__ void split_f32_kernel(const float* __restrict__ x, half_t* __restrict__ y, size_t n8, int C8,
                                 unsigned* __restrict__ ovf) {
  typedef float f4 __attribute__((ext_vector_type(4)));
  typedef _Float16 h8 __attribute__((ext_vector_type(8)));
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n8) return;
  const size_t pix = i / C8;
  const int c = (int)(i - pix * C8) * 8;
  const f4 a = *(const f4*)(x + i * 8), b = *(const f4*)(x + i * 8 + 4);
  const float v[8] = {a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
  h8 h, l;
  bool bad = false;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    h[e] = (half_t)v[e];
    l[e] = (half_t)((v[e] - (float)h[e]) * kSplitLoScale);
    bad = bad || !(__builtin_fabsf(v[e]) <= 65504.f);
  }
  half_t* d = y + pix * (size_t)(16 * C8) + c;
  *(h8*)d = h;
  *(h8*)(d + 8 * C8) = l;
  if (bad && ovf) *ovf = 1u;
}
__global__ void unsplit_f32_kernel(const half_t* __restrict__ x, float* __restrict__ y, size_t n8, int C8) {
  typedef float f4 __attribute__((ext_vector_type(4)));
  typedef _Float16 h8 __attribute__((ext_vector_type(8)));
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n8) return;
  const size_t pix = i / C8;
  const int c = (int)(i - pix * C8) * 8;
  const half_t* sp = x + pix * (size_t)(16 * C8) + c;
  const h8 h = *(const h8*)sp, l = *(const h8*)(sp + 8 * C8);
  f4 a, b;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    a[e] = (float)h[e] + (float)l[e] * kSplitLoInv;
    b[e] = (float)h[e + 4] + (float)l[e + 4] * kSplitLoInv;
  }
  *(f4*)(y + i * 8) = a;
  *(f4*)(y + i * 8 + 4) = b;
}
int launch_split_f32(const float* x, void* y, size_t npix, int C, unsigned* ovf, hipStream_t st) {
  if (C <= 0 || C % 8 || ((uintptr_t)x | (uintptr_t)y) % 16) return kErrArg;
  const size_t n8 = npix * (size_t)(C / 8);
  if (n8 == 0) return kOk;
  if ((n8 + 255) / 256 > 0x7fffffffull) return kErrShape;
  hipLaunchKernelGGL(split_f32_kernel, dim3((unsigned)((n8 + 255) / 256)), dim3(256), 0, st, x, (half_t*)y, n8, C / 8, ovf);
  return (int)hipGetLastError();
}
int launch_unsplit_f32(const void* x, float* y, size_t npix, int C, hipStream_t st) {
  if (C <= 0 || C % 8 || ((uintptr_t)x | (uintptr_t)y) % 16) return kErrArg;
  const size_t n8 = npix * (size_t)(C / 8);
  if (n8 == 0) return kOk;
  if ((n8 + 255) / 256 > 0x7fffffffull) return kErrShape;
  hipLaunchKernelGGL(unsplit_f32_kernel, dim3((unsigned)((n8 + 255) / 256)), dim3(256), 0, st, (const half_t*)x, y, n8, C / 8);
  return (int)hipGetLastError();
}

const char kSwitchRegion[] = "UPR_FP32_SPLIT";

// The five switches and their values.  The three on / off switches are on
// unless set to a number equal to 0 (unset and empty count as on).
//   UPR_FP32_SPLIT       0: every op on the fp32 MFMA kernels (split state 0)
//   UPR_FP32_SPLIT_REGS  0: the split-in-registers ops stay on them, the region stays split
//   UPR_FP32_SPLIT_W64   0: the weights-split-once ops (the 64-wide convs at half resolution) stay on them
//   UPR_RING_SPLIT_LDS   where the ring programs split their activations (the same
//                        bits every way): unset or empty -> each program's default, once
//                        per ring element in LDS; 0 -> once per tap in registers; 2 / 3 ->
//                        every program at the top of the step / one step ahead; anything
//                        else -> the default
//   UPR_W64_RING         0: the 64 -> 64 weights-split-once ops stay on the gathered tile
// (atoi: text that is no number counts as 0)
SplitSwitches read_split_switches() {
  auto on = [](const char* name) {
    const char* e = getenv(name);
    return !(e && *e && atoi(e) == 0);
  };
  SplitSwitches s;
  s.region = on(kSwitchRegion);
  s.regs = on("UPR_FP32_SPLIT_REGS");
  s.w64 = on("UPR_FP32_SPLIT_W64");
  s.ring_split = kRingSplitDefault;
  const char* e = getenv("UPR_RING_SPLIT_LDS");
  if (e && *e) {
    const int v = atoi(e);
    s.ring_split = v == 0 ? kRingSplitTap : v == 2 ? kRingSplitTop : v == 3 ? kRingSplitAhead : kRingSplitDefault;
  }
  s.w64_tile = !on("UPR_W64_RING");
  return s;
}

}  // namespace upr
