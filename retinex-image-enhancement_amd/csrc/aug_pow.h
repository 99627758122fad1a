// x^g for the augmentation's gamma stage (x >= 1e-8 after the clamp, fp32 in
// and out), evaluated in fp64: gfx950 runs fp64 FMAs at the plain fp32 rate,
// and ~45 of them replace the several hundred fp32 instructions of the
// library powf, which made both the statistics and the apply pass ALU-bound
// (profiles/aug_bench_v1.json against _v2).  Only IEEE-exact operations (+, *,
// /, fma, rint, ldexp, conversions), so the host and the device give the same
// bits and the two passes agree with each other.
//
// x = m 2^e with m in [sqrt(1/2), sqrt(2)); log2(m) = (2 / ln 2) atanh(s),
// s = (m - 1) / (m + 1), |s| <= 0.1716, the odd series through s^15 (next
// term 6e-15); t = g (e + log2 m) = n + f; 2^f = exp(f ln 2) by its Taylor
// series through degree 10 (|f ln 2| <= 0.3466, next term 2e-13).  The fp64
// value is within 1e-12 relative of x^g, so the fp32 result is the correctly
// rounded one except within that distance of a rounding boundary.
#pragma once
#include <math.h>

#ifndef __HIPCC__
#define __host__
#define __device__
#endif

__host__ __device__ inline float aug_pow(float x, float g) {
  int e;
  float m = frexpf(x, &e);  // [0.5, 1)
  if (m < 0.70710678f) {
    m *= 2.f;
    e -= 1;
  }
  const double md = (double)m;
  const double s = (md - 1.0) / (md + 1.0), s2 = s * s;
  double p = 1.0 / 15.0;
  p = fma(p, s2, 1.0 / 13.0);
  p = fma(p, s2, 1.0 / 11.0);
  p = fma(p, s2, 1.0 / 9.0);
  p = fma(p, s2, 1.0 / 7.0);
  p = fma(p, s2, 1.0 / 5.0);
  p = fma(p, s2, 1.0 / 3.0);
  p = fma(p, s2, 1.0);
  const double log2m = 2.8853900817779268 * (s * p);  // 2 / ln 2
  const double t = fmin(fmax((double)g * ((double)e + log2m), -1100.0), 1100.0);
  const double n = rint(t);
  const double u = (t - n) * 0.69314718055994531;  // ln 2
  double q = 1.0 / 3628800.0;
  q = fma(q, u, 1.0 / 362880.0);
  q = fma(q, u, 1.0 / 40320.0);
  q = fma(q, u, 1.0 / 5040.0);
  q = fma(q, u, 1.0 / 720.0);
  q = fma(q, u, 1.0 / 120.0);
  q = fma(q, u, 1.0 / 24.0);
  q = fma(q, u, 1.0 / 6.0);
  q = fma(q, u, 0.5);
  q = fma(q, u, 1.0);
  q = fma(q, u, 1.0);
  return (float)ldexp(q, (int)n);
}
