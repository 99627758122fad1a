// Entry and exit kernels of the batched directory harness (gfx950): pure
// streaming, 4 consecutive pixels of one row per lane.
//
//  letterbox_batch  B ragged u8 HWC sources -> one [B,3,Ho,Wo] batch tensor in
//                   one launch; letterbox_kernel's src_kind 0 arithmetic
//                   (enhance.hip), float32 or its fp16 rounding
//  panels_u8        x / enhanced / illumination [B,C,H,W] -> the u8 HWC pixels
//                   of the three output files (to_u8_hwc_kernel's bytes; the
//                   comparison's panels side by side) in one pass
//
// Both launch dim3(row strips, images) blocks of 256 threads = RY rows x TX
// lanes (TX = 64 / 128 / 256 by row length), so a wave stays inside one row:
// per-row terms are loaded once per row and neighbouring lanes hold
// neighbouring pixel groups.
#include <algorithm>

#include "upr_common.h"
#include "../../include/upr.h"

namespace upr {
namespace {

constexpr int kRowsPerBlock = 8;

// as in enhance.hip: numpy's (np.float32 x * 255).astype(np.uint8) on x86-64
__device__ __forceinline__ int quant_u8(float v) {
  const float t = __fmul_rn(v, 255.f);
  if (!(fabsf(t) < 2147483648.f)) return 0;  // NaN, inf, out of int32 range
  return ((int)t) & 255;                      // trunc toward zero, wrap
}
__device__ __forceinline__ int sat_u8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

typedef _Float16 h4_t __attribute__((ext_vector_type(4)));

// 4 consecutive elements: one 16-byte (float) / 8-byte (half) access when the
// address allows it, element by element otherwise (rows of a width that is no
// multiple of 4 start misaligned)
__device__ __forceinline__ void load4(const float* p, float (&v)[4]) {
  if (((uintptr_t)p & 15) == 0) {
    const float4 q = *(const float4*)p;
    v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = p[k];
  }
}
__device__ __forceinline__ void load4(const half_t* p, float (&v)[4]) {
  if (((uintptr_t)p & 7) == 0) {
    const h4_t q = *(const h4_t*)p;
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = (float)q[k];
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = (float)p[k];
  }
}
// the first n (1..4) of 4 values
__device__ __forceinline__ void store4(float* p, const float (&v)[4], int n) {
  if (n == 4 && ((uintptr_t)p & 15) == 0) {
    *(float4*)p = make_float4(v[0], v[1], v[2], v[3]);
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (k < n) p[k] = v[k];
  }
}
__device__ __forceinline__ void store4(half_t* p, const float (&v)[4], int n) {
  if (n == 4 && ((uintptr_t)p & 7) == 0) {
    h4_t q;
#pragma unroll
    for (int k = 0; k < 4; ++k) q[k] = (half_t)v[k];
    *(h4_t*)p = q;
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (k < n) p[k] = (half_t)v[k];
  }
}

// ---------------------------------------------------------------------------
// letterbox_batch.  Image b's record gives its source, tap tables and
// placement; every image lands on the same Ho x Wo canvas.  A lane makes the
// pixels x .. x + 3 of one row.  Without tables (no resize) a group that lies
// inside the image is 12 contiguous source bytes: they are read as the 3 or 4
// aligned dwords that hold them (a dword holding one of the image's bytes lies
// inside the image's pages) and shifted into place, not as 12 byte loads.
// ---------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void letterbox_batch_kernel(const upr_letterbox_rec* __restrict__ recs, int Ho, int Wo,
                                                              int color, T* __restrict__ out, int tx_lanes) {
  const upr_letterbox_rec r = recs[blockIdx.y];
  const int tx = threadIdx.x & (tx_lanes - 1), ty = threadIdx.x / tx_lanes, ry = 256 / tx_lanes;
  const int QW = (Wo + 3) >> 2;
  const size_t plane = (size_t)Ho * Wo;
  T* img = out + (size_t)blockIdx.y * 3 * plane;
  const int yend = min(Ho, ((int)blockIdx.x + 1) * kRowsPerBlock);
  const bool taps = r.xtab != nullptr;
  for (int y = blockIdx.x * kRowsPerBlock + ty; y < yend; y += ry) {
    const int yy = y - r.top;
    const bool yin = yy >= 0 && yy < r.nh;
    int y0 = 0, y1 = 0, b0 = 0, b1 = 0;  // the row's vertical taps, once per row
    if (yin && taps) { y0 = r.ytab[yy]; y1 = r.ytab[r.nh + yy]; b0 = r.ytab[2 * r.nh + yy]; b1 = r.ytab[3 * r.nh + yy]; }
    for (int q = tx; q < QW; q += tx_lanes) {
      const int x = 4 * q, xx = x - r.left;
      int v[3][4];
#pragma unroll
      for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int k = 0; k < 4; ++k) v[c][k] = (color >> (8 * c)) & 255;
      if (yin && xx + 3 >= 0 && xx < r.nw) {
        if (!taps) {
          const uint8_t* p = r.src + ((size_t)yy * r.W + max(xx, 0)) * 3;
          if (xx >= 0 && xx + 3 < r.nw) {
            const unsigned s = (unsigned)((uintptr_t)p & 3);
            const uint32_t* d = (const uint32_t*)(p - s);
            const uint32_t d0 = d[0], d1 = d[1], d2 = d[2], d3 = s ? d[3] : 0u;
            const uint32_t w[3] = {__builtin_amdgcn_alignbyte(d1, d0, s), __builtin_amdgcn_alignbyte(d2, d1, s),
                                   __builtin_amdgcn_alignbyte(d3, d2, s)};
#pragma unroll
            for (int k = 0; k < 4; ++k)
#pragma unroll
              for (int c = 0; c < 3; ++c) v[c][k] = (w[(3 * k + c) >> 2] >> (8 * ((3 * k + c) & 3))) & 255;
          } else {  // a group across the image's left or right edge
#pragma unroll
            for (int k = 0; k < 4; ++k) {
              const int xk = xx + k;
              if (xk >= 0 && xk < r.nw) {
                const uint8_t* s = r.src + ((size_t)yy * r.W + xk) * 3;
#pragma unroll
                for (int c = 0; c < 3; ++c) v[c][k] = s[c];
              }
            }
          }
        } else {
          const uint8_t* r0p = r.src + (size_t)y0 * r.W * 3;
          const uint8_t* r1p = r.src + (size_t)y1 * r.W * 3;
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            const int xk = xx + k;
            if (xk >= 0 && xk < r.nw) {
              const int x0 = r.xtab[xk] * 3, x1 = r.xtab[r.nw + xk] * 3;
              const int a0 = r.xtab[2 * r.nw + xk], a1 = r.xtab[3 * r.nw + xk];
#pragma unroll
              for (int c = 0; c < 3; ++c) {
                const int h0 = (r0p[x0 + c] * a0 + r0p[x1 + c] * a1) >> 4;
                const int h1 = (r1p[x0 + c] * a0 + r1p[x1 + c] * a1) >> 4;
                const int s = ((h0 * b0) >> 16) + ((h1 * b1) >> 16);
                v[c][k] = sat_u8((s + 2) >> 2);
              }
            }
          }
        }
      }
      const int n = min(4, Wo - x);
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        float f[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) f[k] = (float)v[c][k] / 255.f;
        store4(img + c * plane + (size_t)y * Wo + x, f, n);
      }
    }
  }
}

// ---------------------------------------------------------------------------
// panels_u8.  A lane turns 4 pixels into 12 output bytes per destination.
// Where the 12 bytes start on a dword they are three dword stores.  Where
// they start s bytes past one (a row of the comparison starts panel * 3W bytes
// into its line) the lanes of a wave still write whole aligned dwords: lane i
// takes the last s bytes of lane i - 1 (one shuffle) in front of its own and
// stores the three dwords from s bytes before its start; only the first lane
// of a wave writes its leading 4 - s bytes, and the last lane of a run its
// trailing s bytes, one at a time.  No dword store holds a byte of another
// lane's that the other lane also writes.
// ---------------------------------------------------------------------------
__device__ __forceinline__ uint32_t clamp_byte(float v) { return (uint32_t)quant_u8(fminf(fmaxf(v, 0.f), 1.f)); }

// the 12 bytes of 4 RGB pixels, in memory order
__device__ __forceinline__ void pack12(const float (&r)[4], const float (&g)[4], const float (&b)[4], uint32_t (&w)[3]) {
  uint32_t q[12];
#pragma unroll
  for (int k = 0; k < 4; ++k) { q[3 * k] = clamp_byte(r[k]); q[3 * k + 1] = clamp_byte(g[k]); q[3 * k + 2] = clamp_byte(b[k]); }
#pragma unroll
  for (int j = 0; j < 3; ++j) w[j] = q[4 * j] | q[4 * j + 1] << 8 | q[4 * j + 2] << 16 | q[4 * j + 3] << 24;
}

// every lane of the wave calls it (the shuffle); p: where this lane's 12 bytes
// go (p % 4 is the same for the lanes of a row), act: the lane has pixels,
// last: the next lane has none
__device__ __forceinline__ void put12(uint8_t* p, const uint32_t (&w)[3], bool act, bool last) {
  const unsigned s = (unsigned)((uintptr_t)p & 3);
  if (s == 0) {
    if (act) {
      uint32_t* d = (uint32_t*)p;
      d[0] = w[0]; d[1] = w[1]; d[2] = w[2];
    }
    return;
  }
  const uint32_t prev = (uint32_t)__shfl_up((int)w[2], 1, 64);
  if (!act) return;
  const unsigned sh = 4 - s;
  uint32_t* d = (uint32_t*)(p - s);
  if ((threadIdx.x & 63) == 0) {
    for (unsigned i = 0; i < sh; ++i) p[i] = (uint8_t)(w[0] >> (8 * i));
  } else {
    d[0] = __builtin_amdgcn_alignbyte(w[0], prev, sh);
  }
  d[1] = __builtin_amdgcn_alignbyte(w[1], w[0], sh);
  d[2] = __builtin_amdgcn_alignbyte(w[2], w[1], sh);
  if (last)
    for (unsigned i = 0; i < s; ++i) p[12 - s + i] = (uint8_t)(w[2] >> (8 * (sh + i)));
}

__device__ __forceinline__ void put_pixel(uint8_t* p, uint32_t r, uint32_t g, uint32_t b) {
  p[0] = (uint8_t)r; p[1] = (uint8_t)g; p[2] = (uint8_t)b;
}

template <typename T>
__global__ __launch_bounds__(256) void panels_u8_kernel(const T* __restrict__ x, const T* __restrict__ enh,
                                                        const T* __restrict__ illu, int H, int W,
                                                        uint8_t* __restrict__ enh_u8, uint8_t* __restrict__ illu_u8,
                                                        uint8_t* __restrict__ cmp_u8, int P, int tx_lanes) {
  const int tx = threadIdx.x & (tx_lanes - 1), ty = threadIdx.x / tx_lanes, ry = 256 / tx_lanes;
  const int b = blockIdx.y;
  const int nq = W >> 2;
  const size_t HW = (size_t)H * W;
  const int yend = min(H, ((int)blockIdx.x + 1) * kRowsPerBlock);
  for (int y = blockIdx.x * kRowsPerBlock + ty; y < yend; y += ry) {
    const size_t row1 = ((size_t)b * H + y) * W;                 // the row's first pixel in a [B,H,W] map
    const size_t row3 = ((size_t)b * 3 * H + y) * W;             // ... in channel 0 of a [B,3,H,W] tensor
    uint8_t* er = enh_u8 + row1 * 3;
    uint8_t* ir = illu_u8 ? illu_u8 + row1 * 3 : nullptr;
    uint8_t* cr = cmp_u8 ? cmp_u8 + row1 * 3 * P : nullptr;      // panel p's row: + p * 3W
    const bool need_i = ir || (cr && P == 3);
    for (int q0 = 0; q0 < nq; q0 += tx_lanes) {
      const int q = q0 + tx, px = 4 * q;
      const bool act = q < nq, last = q == nq - 1 || (threadIdx.x & 63) == 63;
      uint32_t we[3] = {0u, 0u, 0u}, wi[3] = {0u, 0u, 0u}, wx[3] = {0u, 0u, 0u};
      if (act) {
        float r[4], g[4], bl[4];
        load4(enh + row3 + px, r); load4(enh + row3 + HW + px, g); load4(enh + row3 + 2 * HW + px, bl);
        pack12(r, g, bl, we);
        if (need_i) { load4(illu + row1 + px, r); pack12(r, r, r, wi); }
        if (cr) { load4(x + row3 + px, r); load4(x + row3 + HW + px, g); load4(x + row3 + 2 * HW + px, bl); pack12(r, g, bl, wx); }
      }
      put12(er + 3 * (size_t)px, we, act, last);
      if (ir) put12(ir + 3 * (size_t)px, wi, act, last);
      if (cr) {
        put12(cr + 3 * (size_t)px, wx, act, last);
        put12(cr + 3 * ((size_t)W + px), we, act, last);
        if (P == 3) put12(cr + 3 * (2 * (size_t)W + px), wi, act, last);
      }
    }
    const int px = 4 * nq + tx;  // the row's last W % 4 pixels, one lane each
    if (px < W) {
      const uint32_t e0 = clamp_byte((float)enh[row3 + px]), e1 = clamp_byte((float)enh[row3 + HW + px]),
                     e2 = clamp_byte((float)enh[row3 + 2 * HW + px]);
      const uint32_t iv = need_i ? clamp_byte((float)illu[row1 + px]) : 0u;
      put_pixel(er + 3 * (size_t)px, e0, e1, e2);
      if (ir) put_pixel(ir + 3 * (size_t)px, iv, iv, iv);
      if (cr) {
        put_pixel(cr + 3 * (size_t)px, clamp_byte((float)x[row3 + px]), clamp_byte((float)x[row3 + HW + px]),
                  clamp_byte((float)x[row3 + 2 * HW + px]));
        put_pixel(cr + 3 * ((size_t)W + px), e0, e1, e2);
        if (P == 3) put_pixel(cr + 3 * (2 * (size_t)W + px), iv, iv, iv);
      }
    }
  }
}

// lanes along a row: the smallest of 64 / 128 / 256 that covers `groups`
int row_lanes(int groups) { return groups <= 64 ? 64 : (groups <= 128 ? 128 : 256); }

}  // namespace

int launch_letterbox_batch(const upr_letterbox_rec* recs, int B, int Ho, int Wo, int color, void* out, int dtype,
                           hipStream_t st) {
  const dim3 grid(cdiv(Ho, kRowsPerBlock), B);
  const int lanes = row_lanes((Wo + 3) / 4);
  if (dtype == kF16)
    hipLaunchKernelGGL((letterbox_batch_kernel<half_t>), grid, dim3(256), 0, st, recs, Ho, Wo, color, (half_t*)out,
                       lanes);
  else
    hipLaunchKernelGGL((letterbox_batch_kernel<float>), grid, dim3(256), 0, st, recs, Ho, Wo, color, (float*)out,
                       lanes);
  return (int)hipGetLastError();
}

int launch_panels_u8(const void* x, const void* enh, const void* illu, int B, int H, int W, int dtype, uint8_t* enh_u8,
                     uint8_t* illu_u8, uint8_t* cmp_u8, int P, hipStream_t st) {
  const dim3 grid(cdiv(H, kRowsPerBlock), B);
  const int lanes = row_lanes(std::max(W / 4, W % 4));
  if (dtype == kF16)
    hipLaunchKernelGGL((panels_u8_kernel<half_t>), grid, dim3(256), 0, st, (const half_t*)x, (const half_t*)enh,
                       (const half_t*)illu, H, W, enh_u8, illu_u8, cmp_u8, P, lanes);
  else
    hipLaunchKernelGGL((panels_u8_kernel<float>), grid, dim3(256), 0, st, (const float*)x, (const float*)enh,
                       (const float*)illu, H, W, enh_u8, illu_u8, cmp_u8, P, lanes);
  return (int)hipGetLastError();
}

}  // namespace upr
