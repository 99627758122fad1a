// Training-data augmentation on the device (include/upr_train.h upr_augment*):
// the reference's LowLightDataset.__getitem__ after the letterbox
// (datasets/dataset.py:101-183) -- flips, rot90 and the six photometric stages
// of _apply_advanced_augmentation -- for a whole batch in one call.
//
// Geometry is an inverse map per output pixel.  flip(dims=[2]), flip(dims=[1])
// and rot90(k, dims=[1,2]) compose to
//   even k: out[y][x] = in[fy(y)][fx(x)]     (k = 2 toggles both flips)
//   odd  k: out[i][j] = in[fy(j)][fx(i)]     (a transpose plus flips)
// with fy / fx the identity or the reversal of a row / column index
// (aug_geometry).  Even k keeps rows unit-stride: aug_rows_kernel<true> moves
// 16 bytes per lane and channel (hflip reverses the lanes of a quad and the quad
// order), <false> is the scalar form for W % 4 != 0 or misaligned pointers.
// Odd k goes through a 32 x 32 LDS tile per channel (rows padded to 33 floats:
// the row-wise stores and the column-wise reads are both conflict-free), so
// the global reads and writes both stay coalesced; with H % 4 == 0 the store
// side also works on quads (16-byte stores, one generator call per channel and
// quad, as on the row path).  Offsets inside an image
// are 32-bit (the entry refuses 3*H*W >= 2^31); the per-image base is uniform.
//
// The photometric chain runs on the three channels of a pixel at once (the
// saturation stage mixes them) between the load and the single store; a stage
// whose flag bit is off is skipped.  The contrast stage's per-(image, channel)
// mean of the post-gamma image comes from a statistics pass that runs only
// when some image has contrast on: per-block fp64 partials in the workspace,
// added in a fixed order by aug_stats_fin_kernel, so it is bit-identical run
// to run and nothing persists between calls.
//
// Noise: counter-based Philox4x32-10, key = the call's seed, counter =
// (sample id, element group) with the group = ((c*Ho + y)*Wo + x) / 4 in
// OUTPUT coordinates; the four outputs give four normals by Box-Muller, element
// e of the group takes normal e.  A sample's noise depends on (seed, sample id,
// c, y, x) only.
//
// Built with -ffp-contract=off (csrc/Makefile): the chain's rounding is the
// reference's op-by-op fp32 rounding, whatever path a pixel takes.
#include "upr_common.h"
#include "aug_pow.h"
#include "../../include/upr_train.h"

namespace upr {
namespace {

constexpr int kAugTile = 32;
constexpr int kStatChunk = 4096;  // elements of one plane per statistics block

struct AugGeom {
  int odd;     // rot k odd: the output is [W][H]
  int fy, fx;  // reverse the source row / column index
};

__host__ __device__ inline AugGeom aug_geometry(uint32_t flags) {
  const int hf = flags & UPR_AUG_HFLIP ? 1 : 0, vf = flags & UPR_AUG_VFLIP ? 1 : 0;
  const int k = (flags >> UPR_AUG_ROT_SHIFT) & 3;
  AugGeom g;
  g.odd = k & 1;
  if (k == 0) { g.fy = vf; g.fx = hf; }
  else if (k == 2) { g.fy = vf ^ 1; g.fx = hf ^ 1; }
  else if (k == 1) { g.fy = vf; g.fx = hf ^ 1; }
  else { g.fy = vf ^ 1; g.fx = hf; }
  return g;
}

struct U4 { uint32_t x, y, z, w; };

__device__ __forceinline__ U4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                            uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    const uint32_t n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
    c0 = n0; c1 = lo1; c2 = n2; c3 = lo0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return U4{c0, c1, c2, c3};
}

// two uniforms u = ((r >> 9) + 0.5) 2^-23 in (0, 1), exact in fp32 -> two normals
__device__ __forceinline__ void box_muller(uint32_t a, uint32_t b, float& z0, float& z1) {
  const float u1 = ((float)(a >> 9) + 0.5f) * (1.0f / 8388608.0f);
  const float u2 = ((float)(b >> 9) + 0.5f) * (1.0f / 8388608.0f);
  const float r = sqrtf(-2.0f * logf(u1));
  float s, c;
  sincospif(2.0f * u2, &s, &c);
  z0 = r * c;
  z1 = r * s;
}

// the four normals of one element group of one sample
__device__ __forceinline__ void aug_normals4(uint64_t seed, uint64_t sid, uint32_t group, float (&z)[4]) {
  const U4 r = philox4x32_10((uint32_t)sid, (uint32_t)(sid >> 32), group, 0u, (uint32_t)seed, (uint32_t)(seed >> 32));
  box_muller(r.x, r.y, z[0], z[1]);
  box_muller(r.z, r.w, z[2], z[3]);
}

// the normal of one element (index idx = (c*Ho + y)*Wo + x)
__device__ __forceinline__ float aug_normal1(uint64_t seed, uint64_t sid, uint32_t idx) {
  const U4 r = philox4x32_10((uint32_t)sid, (uint32_t)(sid >> 32), idx >> 2, 0u, (uint32_t)seed,
                             (uint32_t)(seed >> 32));
  float z0, z1;
  if (idx & 2) box_muller(r.z, r.w, z0, z1);
  else box_muller(r.x, r.y, z0, z1);
  return idx & 1 ? z1 : z0;
}

__device__ __forceinline__ float clamp01(float v) { return fminf(fmaxf(v, 0.f), 1.f); }

// pow(clamp(x, min=1e-8), gamma); aug_pow.h: fp64 FMAs instead of the library powf
__device__ __forceinline__ float aug_gamma(float v, float gamma) { return aug_pow(fmaxf(v, 1e-8f), gamma); }

// the six stages on one pixel's three channels, in the reference order
// (dataset.py:133-161); n = this pixel's three normals (read when noise is on)
__device__ __forceinline__ void aug_chain(float (&v)[3], const UprAugParams& p, const float* __restrict__ mean,
                                          const float (&n)[3]) {
  const uint32_t f = p.flags;
  if (f & UPR_AUG_GAMMA) {
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = aug_gamma(v[c], p.gamma);
  }
  if (f & UPR_AUG_CONTRAST) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float m = mean[c];
      v[c] = clamp01((v[c] - m) * p.contrast + m);
    }
  }
  if (f & UPR_AUG_BRIGHTNESS) {
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = clamp01(v[c] + p.brightness);
  }
  if (f & UPR_AUG_NOISE) {
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = clamp01(v[c] + n[c] * p.noise_level);
  }
  if (f & UPR_AUG_SATURATION) {
    const float gray = (0.299f * v[0] + 0.587f * v[1]) + 0.114f * v[2];
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = clamp01(gray + p.saturation * (v[c] - gray));
  }
  if (f & UPR_AUG_SHIFT) {
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = clamp01(v[c] + p.shift);
  }
}

// ---- statistics pass: per-(image, channel) sum of the post-gamma image ------
// grid (nblk, 3, B); block k of a plane sums elements [k*kStatChunk, +kStatChunk)
// into part[(b*3 + c)*nblk + k].  Images without contrast write nothing.
template <bool VEC>
__global__ __launch_bounds__(256) void aug_stats_kernel(const float* __restrict__ x,
                                                        const UprAugParams* __restrict__ params,
                                                        double* __restrict__ part, int HW, int nblk) {
  __shared__ double red[4];
  const int b = blockIdx.z, c = blockIdx.y, t = threadIdx.x;
  const UprAugParams p = params[b];
  if (!(p.flags & UPR_AUG_CONTRAST)) return;
  const bool gam = p.flags & UPR_AUG_GAMMA;
  const float* xp = x + ((size_t)b * 3 + c) * HW;
  const int base = blockIdx.x * kStatChunk;
  double a = 0.0;
  if (VEC) {
#pragma unroll
    for (int k = 0; k < kStatChunk / 1024; ++k) {
      const int i = base + (k * 256 + t) * 4;
      if (i < HW) {  // HW % 4 == 0: a quad is whole or absent
        const float4 q = *(const float4*)(xp + i);
        float v[4] = {q.x, q.y, q.z, q.w};
        if (gam) {
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = aug_gamma(v[e], p.gamma);
        }
        a += ((double)v[0] + (double)v[1]) + ((double)v[2] + (double)v[3]);
      }
    }
  } else {
    // the same elements per thread and the same order of additions as above, so
    // the mean does not depend on which form ran (an absent element adds 0)
#pragma unroll
    for (int k = 0; k < kStatChunk / 1024; ++k) {
      const int i = base + (k * 256 + t) * 4;
      double d[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float v = 0.f;
        if (i + e < HW) {
          v = xp[i + e];
          if (gam) v = aug_gamma(v, p.gamma);
        }
        d[e] = (double)v;
      }
      a += (d[0] + d[1]) + (d[2] + d[3]);
    }
  }
  // fixed xor tree within each wave, then the 4 wave sums in order
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o, 64);
  if ((t & 63) == 0) red[t >> 6] = a;
  __syncthreads();
  if (t == 0) part[((size_t)b * 3 + c) * nblk + blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

// grid (3, B): thread t adds partials t, t + 256, ... then the same fixed tree
__global__ __launch_bounds__(256) void aug_stats_fin_kernel(const double* __restrict__ part,
                                                            const UprAugParams* __restrict__ params,
                                                            float* __restrict__ mean, int HW, int nblk) {
  __shared__ double red[4];
  const int b = blockIdx.y, c = blockIdx.x, t = threadIdx.x;
  if (!(params[b].flags & UPR_AUG_CONTRAST)) return;
  const double* pp = part + ((size_t)b * 3 + c) * nblk;
  double a = 0.0;
  for (int i = t; i < nblk; i += 256) a += pp[i];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o, 64);
  if ((t & 63) == 0) red[t >> 6] = a;
  __syncthreads();
  if (t == 0) mean[b * 3 + c] = (float)((((red[0] + red[1]) + red[2]) + red[3]) / (double)HW);
}

// the rest of a pixel's / a quad's way after the gather: its normals (the caller's
// noise tensor or the generator), the chain, one store per channel.  oo = the
// offset in the output plane; a quad starts at oo % 4 == 0 with HW % 4 == 0,
// so it is exactly one element group of the generator per channel.
__device__ __forceinline__ void aug_finish_px(float (&v)[3], const UprAugParams& p, const float* __restrict__ mb,
                                              const float* __restrict__ nb, uint64_t seed, int HW, int oo,
                                              float* __restrict__ yb) {
  float n[3] = {0.f, 0.f, 0.f};
  if (p.flags & UPR_AUG_NOISE) {
#pragma unroll
    for (int c = 0; c < 3; ++c) n[c] = nb ? nb[c * HW + oo] : aug_normal1(seed, p.sample_id, (uint32_t)(c * HW + oo));
  }
  aug_chain(v, p, mb, n);
#pragma unroll
  for (int c = 0; c < 3; ++c) yb[c * HW + oo] = v[c];
}

__device__ __forceinline__ void aug_finish_quad(float (&v)[4][3], const UprAugParams& p,
                                                const float* __restrict__ mb, const float* __restrict__ nb,
                                                uint64_t seed, int HW, int oo, float* __restrict__ yb) {
  float n[4][3] = {};
  if (p.flags & UPR_AUG_NOISE) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      float z[4];
      if (nb) {
        const float4 q = *(const float4*)(nb + c * HW + oo);
        z[0] = q.x; z[1] = q.y; z[2] = q.z; z[3] = q.w;
      } else {
        aug_normals4(seed, p.sample_id, (uint32_t)(c * HW + oo) >> 2, z);
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) n[e][c] = z[e];
    }
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) aug_chain(v[e], p, mb, n[e]);
#pragma unroll
  for (int c = 0; c < 3; ++c) *(float4*)(yb + c * HW + oo) = make_float4(v[0][c], v[1][c], v[2][c], v[3][c]);
}

// ---- apply pass, even k: unit-stride rows -----------------------------------
// grid (cdiv(units, 256), B); a unit is a quad of 4 output pixels (VEC) or one
// output pixel.  Images with odd k are left to aug_transpose_kernel.
template <bool VEC>
__global__ __launch_bounds__(256) void aug_rows_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                       const UprAugParams* __restrict__ params,
                                                       const float* __restrict__ mean,
                                                       const float* __restrict__ noise, uint64_t seed, int H, int W) {
  const int b = blockIdx.y;
  const UprAugParams p = params[b];
  const AugGeom g = aug_geometry(p.flags);
  if (g.odd) return;
  const int HW = H * W;
  const float* xb = x + (size_t)b * 3 * HW;
  float* yb = y + (size_t)b * 3 * HW;
  const float* nb = noise ? noise + (size_t)b * 3 * HW : nullptr;
  const float* mb = mean + b * 3;
  const int u = blockIdx.x * 256 + threadIdx.x;
  if (VEC) {
    const int qpr = W >> 2;
    if (u >= qpr * H) return;
    const int oy = u / qpr, ox = (u - oy * qpr) * 4;
    const int sy = g.fy ? H - 1 - oy : oy, sx = g.fx ? W - 4 - ox : ox;
    const int so = sy * W + sx, oo = oy * W + ox;
    float v[4][3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float4 q = *(const float4*)(xb + c * HW + so);
      // hflip: the quad order is reversed by sx, the lanes of the quad here
      v[0][c] = g.fx ? q.w : q.x;
      v[1][c] = g.fx ? q.z : q.y;
      v[2][c] = g.fx ? q.y : q.z;
      v[3][c] = g.fx ? q.x : q.w;
    }
    aug_finish_quad(v, p, mb, nb, seed, HW, oo, yb);
  } else {
    if (u >= HW) return;
    const int oy = u / W, ox = u - oy * W;
    const int sy = g.fy ? H - 1 - oy : oy, sx = g.fx ? W - 1 - ox : ox;
    const int so = sy * W + sx;
    float v[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = xb[c * HW + so];
    aug_finish_px(v, p, mb, nb, seed, HW, u, yb);
  }
}

// ---- apply pass, odd k: LDS tile transpose -----------------------------------
// grid (cdiv(H, 32), cdiv(W, 32), B): block (tj, ti) writes output rows
// i0..i0+31 (of W) x columns j0..j0+31 (of H) of out[W][H] = in[fy(j)][fx(i)].
// Load: lanes run along i (consecutive source columns, reversed under fx);
// store: lanes run along j (consecutive output columns), LDS read column-wise;
// VEC (H % 4 == 0, 16-byte aligned y / noise): a thread takes 4 consecutive j
// of one row, 8 lanes a 128-byte run; its LDS reads hit bank (4q + e + ii) % 32,
// distinct over the 8 quads x 4 rows of a half-wave.
template <bool VEC>
__global__ __launch_bounds__(256) void aug_transpose_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                            const UprAugParams* __restrict__ params,
                                                            const float* __restrict__ mean,
                                                            const float* __restrict__ noise, uint64_t seed, int H,
                                                            int W) {
  __shared__ float tile[3][kAugTile][kAugTile + 1];
  const int b = blockIdx.z;
  const UprAugParams p = params[b];
  const AugGeom g = aug_geometry(p.flags);
  if (!g.odd) return;
  const int HW = H * W;
  const float* xb = x + (size_t)b * 3 * HW;
  float* yb = y + (size_t)b * 3 * HW;
  const float* nb = noise ? noise + (size_t)b * 3 * HW : nullptr;
  const float* mb = mean + b * 3;
  const int j0 = blockIdx.x * kAugTile, i0 = blockIdx.y * kAugTile;
  const int l = threadIdx.x & 31, r0 = threadIdx.x >> 5;
  {
    const int i = i0 + l;  // output row = source column
    const int sx = g.fx ? W - 1 - i : i;
#pragma unroll
    for (int rr = 0; rr < kAugTile; rr += 8) {
      const int jj = rr + r0, j = j0 + jj;  // output column = source row
      if (i < W && j < H) {
        const int so = (g.fy ? H - 1 - j : j) * W + sx;
#pragma unroll
        for (int c = 0; c < 3; ++c) tile[c][jj][l] = xb[c * HW + so];
      }
    }
  }
  __syncthreads();
  if (VEC) {
    const int ii = threadIdx.x >> 3, jq = (threadIdx.x & 7) * 4;
    const int i = i0 + ii, j = j0 + jq;
    if (i < W && j < H) {  // H % 4 == 0: a quad is whole or absent
      float v[4][3];
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int c = 0; c < 3; ++c) v[e][c] = tile[c][jq + e][ii];
      aug_finish_quad(v, p, mb, nb, seed, HW, i * H + j, yb);  // the output image is [W][H]
    }
  } else {
    const int j = j0 + l;
#pragma unroll
    for (int rr = 0; rr < kAugTile; rr += 8) {
      const int ii = rr + r0, i = i0 + ii;
      if (i < W && j < H) {
        float v[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = tile[c][l][ii];
        aug_finish_px(v, p, mb, nb, seed, HW, i * H + j, yb);
      }
    }
  }
}

// ---- debug: the raw normals of B samples, out [B][3*Ho*Wo] ------------------
__global__ __launch_bounds__(256) void aug_normals_kernel(float* __restrict__ out,
                                                          const UprAugParams* __restrict__ params, uint64_t seed,
                                                          int n) {
  const int b = blockIdx.y;
  const int grp = blockIdx.x * 256 + threadIdx.x;
  if (grp * 4 >= n) return;
  float z[4];
  aug_normals4(seed, params[b].sample_id, (uint32_t)grp, z);
  float* ob = out + (size_t)b * n + grp * 4;
#pragma unroll
  for (int e = 0; e < 4; ++e)
    if (grp * 4 + e < n) ob[e] = z[e];
}

inline int aug_stat_blocks(int H, int W) { return cdiv(H * W, kStatChunk); }
inline bool aug_shape_ok(int B, int H, int W) {
  return B >= 1 && B <= 65535 && H >= 1 && W >= 1 && (int64_t)3 * H * W < ((int64_t)1 << 31);
}

}  // namespace
}  // namespace upr

using namespace upr;

extern "C" {

size_t upr_augment_workspace(int B, int H, int W) {
  if (!aug_shape_ok(B, H, W)) return 0;
  return align_up((size_t)B * 3 * aug_stat_blocks(H, W) * sizeof(double), 256) + align_up((size_t)B * 3 * sizeof(float), 256);
}

int upr_augment(const float* x, float* y, int B, int H, int W, const UprAugParams* params,
                const UprAugParams* params_host, uint64_t seed, const float* noise, void* ws, size_t ws_bytes,
                void* stream) {
  if (!x || !y || !params || !params_host || x == y) return kErrArg;
  if (!aug_shape_ok(B, H, W)) return kErrShape;
  // every image must give the same output shape: nothing is launched otherwise
  bool any_odd = false, any_even = false, any_contrast = false;
  for (int b = 0; b < B; ++b) {
    const AugGeom g = aug_geometry(params_host[b].flags);
    (g.odd ? any_odd : any_even) = true;
    any_contrast |= (params_host[b].flags & UPR_AUG_CONTRAST) != 0;
  }
  if (any_odd && any_even && H != W) return kErrShape;
  if (!ws || (uintptr_t)ws % 8 || ws_bytes < upr_augment_workspace(B, H, W)) return kErrWorkspace;
  hipStream_t st = (hipStream_t)stream;
  const int HW = H * W, nblk = aug_stat_blocks(H, W);
  double* part = (double*)ws;
  float* mean = (float*)((char*)ws + align_up((size_t)B * 3 * nblk * sizeof(double), 256));
  const bool xvec = HW % 4 == 0 && (uintptr_t)x % 16 == 0;
  if (any_contrast) {
    if (xvec)
      hipLaunchKernelGGL((aug_stats_kernel<true>), dim3(nblk, 3, B), dim3(256), 0, st, x, params, part, HW, nblk);
    else
      hipLaunchKernelGGL((aug_stats_kernel<false>), dim3(nblk, 3, B), dim3(256), 0, st, x, params, part, HW, nblk);
    UPR_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(aug_stats_fin_kernel, dim3(3, B), dim3(256), 0, st, (const double*)part, params, mean, HW,
                       nblk);
    UPR_CHECK_HIP(hipGetLastError());
  }
  if (any_even) {
    const bool vec = W % 4 == 0 && (uintptr_t)x % 16 == 0 && (uintptr_t)y % 16 == 0 && (uintptr_t)noise % 16 == 0;
    if (vec)
      hipLaunchKernelGGL((aug_rows_kernel<true>), dim3(cdiv(HW / 4, 256), B), dim3(256), 0, st, x, y, params,
                         (const float*)mean, noise, seed, H, W);
    else
      hipLaunchKernelGGL((aug_rows_kernel<false>), dim3(cdiv(HW, 256), B), dim3(256), 0, st, x, y, params,
                         (const float*)mean, noise, seed, H, W);
    UPR_CHECK_HIP(hipGetLastError());
  }
  if (any_odd) {
    const dim3 grid(cdiv(H, kAugTile), cdiv(W, kAugTile), B);
    if (H % 4 == 0 && (uintptr_t)y % 16 == 0 && (uintptr_t)noise % 16 == 0)
      hipLaunchKernelGGL((aug_transpose_kernel<true>), grid, dim3(256), 0, st, x, y, params, (const float*)mean, noise,
                         seed, H, W);
    else
      hipLaunchKernelGGL((aug_transpose_kernel<false>), grid, dim3(256), 0, st, x, y, params, (const float*)mean,
                         noise, seed, H, W);
    UPR_CHECK_HIP(hipGetLastError());
  }
  return kOk;
}

int upr_augment_normals(float* out, int B, int Ho, int Wo, const UprAugParams* params, uint64_t seed, void* stream) {
  if (!out || !params) return kErrArg;
  if (!aug_shape_ok(B, Ho, Wo)) return kErrShape;
  const int n = 3 * Ho * Wo;
  hipLaunchKernelGGL(aug_normals_kernel, dim3(cdiv(cdiv(n, 4), 256), B), dim3(256), 0, (hipStream_t)stream, out,
                     params, seed, n);
  return (int)hipGetLastError();
}

}  // extern "C"
