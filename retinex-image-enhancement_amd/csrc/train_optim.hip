// Optimiser step for gfx950 (reference trainers/train.py:63-103): squared
// gradient norm (fp64 accumulator), GradScaler's unscale, clip + Adam.
// Entries: include/upr_train.h; layout and precision: train_common.h.
#include <cmath>

#include "train_common.h"

namespace upr {

// ---------------------------------------------------------------------------
// optimiser
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sqsum_kernel(const float* __restrict__ g, long long n, double* acc) {
  double v[1] = {0.0};
  GSTRIDE(i, n) v[0] += (double)g[i] * g[i];
  double* dst[1] = {acc};
  block_sum_atomic<1>(v, dst);
}

// GradScaler.unscale_ (torch.amp.GradScaler, train.py:84-86): g *= 1/scale and
// found_inf = 1 if any unscaled value is inf/nan (a benign same-value race)
__global__ __launch_bounds__(256) void unscale_kernel(float* __restrict__ g, long long n,
                                                      const float* __restrict__ scale, float* __restrict__ found_inf) {
  const float inv = 1.f / *scale;
  bool bad = false;
  GSTRIDE(i, n) {
    const float v = g[i] * inv;
    g[i] = v;
    bad |= !isfinite(v);
  }
  if (bad) *found_inf = 1.f;
}

__global__ void adam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                            float* __restrict__ v, long long n, const double* __restrict__ sq, float max_norm,
                            float step, float b1, float b2, float omb1, float omb2, float eps, float wd,
                            float bc2s, float* norm_out) {
  const float norm = (float)sqrt(*sq);
  float coef = 1.f;
  if (max_norm > 0.f) coef = fminf(max_norm / (norm + 1e-6f), 1.f);
  if (norm_out && blockIdx.x == 0 && threadIdx.x == 0) *norm_out = norm;
  GSTRIDE(i, n) {
    const float pv = p[i];
    const float gv = g[i] * coef + wd * pv;
    const float mv = b1 * m[i] + omb1 * gv;
    const float vv = b2 * v[i] + omb2 * gv * gv;
    m[i] = mv;
    v[i] = vv;
    p[i] = pv - step * mv / (sqrtf(vv) / bc2s + eps);
  }
}

}  // namespace upr

using namespace upr;

extern "C" {

int upr_t_sqsum(const float* g, size_t n, double* acc, void* stream) {
  if (!g || !acc) return UPR_ERR_ARG;
  hipLaunchKernelGGL(sqsum_kernel, dim3(grid_for((long long)n, 256, 2048)), dim3(256), 0, ST(stream), g,
                     (long long)n, acc);
  LAUNCH_CHECK();
}

int upr_t_unscale(float* g, size_t n, const float* scale, float* found_inf, void* stream) {
  if (!g || !scale || !found_inf) return UPR_ERR_ARG;
  hipLaunchKernelGGL(unscale_kernel, dim3(grid_for((long long)n, 256, 2048)), dim3(256), 0, ST(stream), g,
                     (long long)n, scale, found_inf);
  LAUNCH_CHECK();
}

int upr_t_adam(float* p, const float* g, float* m, float* v, size_t n, const double* sqsum, float max_norm, float lr,
               double beta1, double beta2, float eps, float weight_decay, int step, float* norm_out, void* stream) {
  if (!p || !g || !m || !v || !sqsum || step <= 0) return UPR_ERR_ARG;
  // torch.optim.Adam keeps the betas, 1 - beta and the bias corrections in
  // double and rounds each once: 1.f - (float)0.999 is 1.3e-5 off 0.001, and
  // so was every v
  const double bc1 = 1.0 - pow(beta1, (double)step);
  const double bc2s = sqrt(1.0 - pow(beta2, (double)step));
  hipLaunchKernelGGL(adam_kernel, dim3(grid_for((long long)n)), dim3(256), 0, ST(stream), p, g, m, v, (long long)n,
                     sqsum, max_norm, (float)((double)lr / bc1), (float)beta1, (float)beta2, (float)(1.0 - beta1),
                     (float)(1.0 - beta2), eps, weight_decay, (float)bc2s, norm_out);
  LAUNCH_CHECK();
}

}  // extern "C"
