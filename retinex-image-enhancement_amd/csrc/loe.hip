// Lightness order error (LOE; Wang, Zheng, Hu, Li, "Naturalness preserved
// enhancement algorithm for non-uniform illumination images", IEEE TIP 2013)
// of an enhanced image against its own low-light input, per image of a batch.
// No reference counterpart: the reference quotes no measure that needs no
// ground truth.  Integer and exact (include/upr.h upr_image_loe):
//   L(p)  = max over R, G, B of the u8 cast of upr_to_u8_hwc (clamp to [0, 1],
//           times 255 in float32, truncated)
//   grid  every pixel when sample == 0 or min(H, W) <= sample, else h x w
//           nearest pixel centres, h = max(1, (H sample + m / 2) / m)
//   D     ordered pairs (x, y) of grid pixels whose order differs:
//           (L_low(x) >= L_low(y)) != (L_enh(x) >= L_enh(y))
//   loe   D / N, N = h w
// The pairs are never visited.  With J[a][b] the joint histogram of (L_low,
// L_enh) over the grid and C its 2-D inclusive prefix, a pixel of bin (a, b)
// has C[a][255] partners y with L_low(y) <= a, C[255][b] with L_enh(y) <= b and
// C[a][b] with both, so D = sum J[a][b] (C[a][255] + C[255][b] - 2 C[a][b]).
//
// loe_hist_kernel (pass 1): every grid pixel of both images is read once and
// counted into the image's 256 x 256 int32 table in the workspace.  All adds
// are integer, so the table does not depend on the order of blocks or lanes.
//   LDS form    a block takes LOE_PPB (16384 < 2^16) consecutive grid pixels
//               and counts them in a private table of 65536 packed 16-bit
//               counters (128 KB of LDS, one block per CU), then adds its
//               non-zero counters to the image's table, lane i of a wave at
//               word i of a 256-byte run.
//   global form one global atomic per pixel: grids of at most LOE_SMALL pixels
//               (a sample = 50 call, unless the image is a long strip), where
//               the few thousand atomics cost no more than zeroing and scanning
//               128 KB of LDS (a tie, 2-3 us faster on
//               flat images).
//   Both forms first ask whether all valid lanes of the wave hold one bin (a
//   flat region: 64 adds to one address would serialise); then one lane adds
//   the lane count.  UPR_LOE_HIST = 1 / 2 forces the LDS / global form (A/B,
//   tools/loe_bench.py).
//   Full grids whose planes are 16-byte aligned (H W a multiple of 4 floats /
//   8 halfs) are read as linear planes with 16-byte loads; other grids pixel
//   by pixel.
// loe_fin_kernel (pass 2): one 1024-thread block per image.  (1) running sums
// down the columns, written to a second table S; (2) a wave per row: the
// inclusive scan of S's row is C[a][.], and the row's share of the dot product
// is added in int64; the row a = 255 also adds sum_b S[255][b] C[255][b], the
// C[255][b] term.  (3) lanes by butterfly, the 16 waves in order (integer sums:
// any order gives the same value), one fp64 division.
#include <cstdlib>

#include "upr_common.h"

namespace upr {

constexpr int LOE_NT = 1024;
constexpr int LOE_PPB = 16384;     // grid pixels per block: below 2^16, the packed counters cannot carry
constexpr int LOE_SMALL = 16384;   // grids up to this many pixels take the global form
constexpr int LOE_BINS = 256 * 256;
static_assert(LOE_PPB < 65536 && LOE_PPB % (8 * LOE_NT) == 0, "16-bit counters; whole 16-byte vectors per thread");

template <typename T>
struct LoeVec;
template <>
struct LoeVec<float> {
  typedef float type __attribute__((ext_vector_type(4)));
  static constexpr int N = 4;
};
template <>
struct LoeVec<half_t> {
  typedef _Float16 type __attribute__((ext_vector_type(8)));
  static constexpr int N = 8;
};

// upr_to_u8_hwc's cast (enhance.hip to_u8_hwc_kernel)
__device__ __forceinline__ int loe_q(float v) {
  const float t = __fmul_rn(fminf(fmaxf(v, 0.f), 1.f), 255.f);
  return (int)t;
}
__device__ __forceinline__ int loe_light(float r, float g, float b) {
  const int qr = loe_q(r), qg = loe_q(g), qb = loe_q(b);
  return qr > qg ? (qr > qb ? qr : qb) : (qg > qb ? qg : qb);
}

// one pixel per lane (valid or not; called by every lane of the wave)
template <bool LDS>
__device__ __forceinline__ void loe_count(unsigned* cnt, int* J, int bin, bool valid, int lane) {
  const unsigned long long m = __ballot(valid);
  if (m == 0) return;  // (wave-uniform)
  const int first = __ffsll((long long)m) - 1;
  const int bin0 = __shfl(bin, first, 64);
  const bool flat = __ballot(valid && bin != bin0) == 0;
  int add = 1;
  if (flat) {
    valid = lane == first;
    add = __popcll(m);
  }
  if (valid) {
    if constexpr (LDS)
      atomicAdd(&cnt[bin >> 1], (unsigned)add << ((bin & 1) * 16));
    else
      atomicAdd(&J[bin], add);
  }
}

template <typename T, bool LDS>
__global__ __launch_bounds__(LOE_NT) void loe_hist_kernel(const T* __restrict__ low, const T* __restrict__ enh,
                                                          int* __restrict__ J, int H, int W, int h, int w, int vec) {
  __shared__ __attribute__((aligned(16))) unsigned cnt[LDS ? LOE_BINS / 2 : 4];
  const int t = threadIdx.x, lane = t & 63;
  const size_t HW = (size_t)H * W;
  const int N = h * w;  // (H W < 2^31)
  const int p0 = blockIdx.x * LOE_PPB;
  const int p1 = N - p0 < LOE_PPB ? N : p0 + LOE_PPB;
  const T* lb = low + (size_t)blockIdx.y * 3 * HW;
  const T* eb = enh + (size_t)blockIdx.y * 3 * HW;
  int* Jb = J + (size_t)blockIdx.y * LOE_BINS;
  if constexpr (LDS) {
    for (int i = t; i < LOE_BINS / 8; i += LOE_NT) ((uint4*)cnt)[i] = make_uint4(0, 0, 0, 0);
    __syncthreads();
  }
  if (vec) {
    // the full grid as linear planes: p0, p1 and H W are multiples of V
    typedef typename LoeVec<T>::type vec_t;
    constexpr int V = LoeVec<T>::N;
    for (int base = p0; base < p1; base += LOE_NT * V) {
      const int p = base + t * V;
      const bool valid = p < p1;
      int bins[V];
      if (valid) {
        vec_t x[3], y[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          x[c] = *(const vec_t*)(lb + c * HW + p);
          y[c] = *(const vec_t*)(eb + c * HW + p);
        }
#pragma unroll
        for (int k = 0; k < V; ++k)
          bins[k] = loe_light((float)x[0][k], (float)x[1][k], (float)x[2][k]) * 256 +
                    loe_light((float)y[0][k], (float)y[1][k], (float)y[2][k]);
      } else {
#pragma unroll
        for (int k = 0; k < V; ++k) bins[k] = 0;
      }
#pragma unroll
      for (int k = 0; k < V; ++k) loe_count<LDS>(cnt, Jb, bins[k], valid, lane);
    }
  } else {
    const bool full = h == H && w == W;
    for (int base = p0; base < p1; base += LOE_NT) {
      const int p = base + t;
      const bool valid = p < p1;
      int bin = 0;
      if (valid) {
        size_t off = (size_t)p;
        if (!full) {
          // nearest pixel centre: grid row i is source row ((2 i + 1) H) / (2 h) < H
          const int i = p / w, j = p - i * w;
          const long long sr = ((2LL * i + 1) * H) / (2LL * h), sc = ((2LL * j + 1) * W) / (2LL * w);
          off = (size_t)sr * W + (size_t)sc;
        }
        bin = loe_light((float)lb[off], (float)lb[HW + off], (float)lb[2 * HW + off]) * 256 +
              loe_light((float)eb[off], (float)eb[HW + off], (float)eb[2 * HW + off]);
      }
      loe_count<LDS>(cnt, Jb, bin, valid, lane);
    }
  }
  if constexpr (LDS) {
    __syncthreads();
    for (int i = t; i < LOE_BINS / 2; i += LOE_NT) {
      const unsigned v = cnt[i];
      if (v & 0xffffu) atomicAdd(&Jb[2 * i], (int)(v & 0xffffu));
      if (v >> 16) atomicAdd(&Jb[2 * i + 1], (int)(v >> 16));
    }
  }
}

__global__ __launch_bounds__(LOE_NT) void loe_fin_kernel(const int* __restrict__ J, int* S, double* __restrict__ loe,
                                                         long long* __restrict__ counts, long long N) {
  __shared__ int qoff[4][256];  // per column: the sum of the row quarters above this one
  __shared__ long long wsum[LOE_NT / 64];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int* Jb = J + (size_t)blockIdx.x * LOE_BINS;
  int* Sb = S + (size_t)blockIdx.x * LOE_BINS;
  // (1) running sums down the columns, a quarter of the rows per thread
  {
    const int q = t >> 8, col = t & 255;
    int s = 0;
    for (int a = q * 64; a < q * 64 + 64; ++a) {
      s += Jb[a * 256 + col];
      Sb[a * 256 + col] = s;
    }
    qoff[q][col] = s;
  }
  __syncthreads();
  if (t < 256) {
    const int s0 = qoff[0][t], s1 = qoff[1][t], s2 = qoff[2][t];
    qoff[0][t] = 0;
    qoff[1][t] = s0;
    qoff[2][t] = s0 + s1;
    qoff[3][t] = (s0 + s1) + s2;
  }
  __syncthreads();  // (also orders this block's stores to S before its loads below)
  // (2) a wave per row, 4 columns per lane
  long long acc = 0;
  for (int a = wave; a < 256; a += LOE_NT / 64) {
    const int4 j = *(const int4*)(Jb + a * 256 + 4 * lane);
    const int4 s = *(const int4*)(Sb + a * 256 + 4 * lane);
    const int* qo = &qoff[a >> 6][4 * lane];
    const int s0 = s.x + qo[0], s1 = s.y + qo[1], s2 = s.z + qo[2], s3 = s.w + qo[3];  // column sums to row a
    int c0 = s0, c1 = c0 + s1, c2 = c1 + s2, c3 = c2 + s3;
    int incl = c3;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int v = __shfl_up(incl, o, 64);
      if (lane >= o) incl += v;
    }
    const int excl = incl - c3;
    c0 += excl;
    c1 += excl;
    c2 += excl;
    c3 += excl;
    const long long rowc = __shfl(incl, 63, 64);  // C[a][255]
    acc += (long long)j.x * (rowc - 2LL * c0) + (long long)j.y * (rowc - 2LL * c1) +
           (long long)j.z * (rowc - 2LL * c2) + (long long)j.w * (rowc - 2LL * c3);
    if (a == 255)  // (wave-uniform) the column totals against C[255][.]
      acc += (long long)s0 * c0 + (long long)s1 * c1 + (long long)s2 * c2 + (long long)s3 * c3;
  }
  // (3)
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
  if (lane == 0) wsum[wave] = acc;
  __syncthreads();
  if (t != 0) return;
  long long D = 0;
  for (int k = 0; k < LOE_NT / 64; ++k) D += wsum[k];
  loe[blockIdx.x] = (double)D / (double)N;
  if (counts) {
    counts[2 * (size_t)blockIdx.x] = D;
    counts[2 * (size_t)blockIdx.x + 1] = N;
  }
}

void loe_grid(int H, int W, int sample, int* h, int* w) {
  const int m = H < W ? H : W;
  if (sample <= 0 || m <= sample) {
    *h = H;
    *w = W;
    return;
  }
  const long long gh = ((long long)H * sample + m / 2) / m, gw = ((long long)W * sample + m / 2) / m;
  *h = gh < 1 ? 1 : (int)gh;
  *w = gw < 1 ? 1 : (int)gw;
}

// the image's table J, then pass 2's column sums S
size_t loe_ws(int B) { return (size_t)B * LOE_BINS * sizeof(int) * 2; }

template <typename T>
static int launch_loe_t(const T* low, const T* enh, double* loe, long long* counts, uint8_t* ws, int B, int H, int W,
                        int sample, hipStream_t st) {
  int h, w;
  loe_grid(H, W, sample, &h, &w);
  const int N = h * w;
  int* J = (int*)ws;
  int* S = J + (size_t)B * LOE_BINS;
  UPR_CHECK_HIP(hipMemsetAsync(J, 0, (size_t)B * LOE_BINS * sizeof(int), st));
  constexpr int V = LoeVec<T>::N;
  const size_t HW = (size_t)H * W;
  const int vec = h == H && w == W && HW % V == 0 && (uintptr_t)low % 16 == 0 && (uintptr_t)enh % 16 == 0;
  // UPR_LOE_HIST: 1 the LDS form for every grid, 2 the global form (A/B); else by the grid's size
  const char* e = getenv("UPR_LOE_HIST");
  const int force = e ? atoi(e) : 0;
  const bool lds = force == 1 || (force != 2 && N > LOE_SMALL);
  // (blockIdx.y carries the image: at most 65535 per launch)
  for (int b0 = 0; b0 < B; b0 += 65535) {
    const int nb = B - b0 < 65535 ? B - b0 : 65535;
    const dim3 grid(cdiv(N, LOE_PPB), nb);
    const T* x = low + (size_t)b0 * 3 * HW;
    const T* y = enh + (size_t)b0 * 3 * HW;
    int* Jp = J + (size_t)b0 * LOE_BINS;
    if (lds)
      hipLaunchKernelGGL((loe_hist_kernel<T, true>), grid, dim3(LOE_NT), 0, st, x, y, Jp, H, W, h, w, vec);
    else
      hipLaunchKernelGGL((loe_hist_kernel<T, false>), grid, dim3(LOE_NT), 0, st, x, y, Jp, H, W, h, w, vec);
    UPR_CHECK_HIP(hipGetLastError());
  }
  hipLaunchKernelGGL(loe_fin_kernel, dim3(B), dim3(LOE_NT), 0, st, J, S, loe, counts, (long long)N);
  UPR_CHECK_HIP(hipGetLastError());
  return kOk;
}

int launch_loe(const void* low, const void* enh, double* loe, long long* counts, uint8_t* ws, int B, int H, int W,
               int sample, int dtype, hipStream_t st) {
  if (dtype == kF16)
    return launch_loe_t((const half_t*)low, (const half_t*)enh, loe, counts, ws, B, H, W, sample, st);
  return launch_loe_t((const float*)low, (const float*)enh, loe, counts, ws, B, H, W, sample, st);
}

}  // namespace upr
