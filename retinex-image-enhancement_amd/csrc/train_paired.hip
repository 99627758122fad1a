// Paired training terms against a ground truth (upr_t_loss_paired): the
// Charbonnier reconstruction term and 1 - mean SSIM, with their gradient w.r.t.
// the enhanced image accumulated into the loss engine's g_enh, in two launches.
//
// The SSIM is the one of utils.utils.calculate_ssim / upr_image_metrics
// (metrics.hip): 11 x 11 box window divided by 121 over a zero border of 5,
// C1 = 0.01^2, C2 = 0.03^2, the map taken at every image position per channel.
// With the window means mx, my, exx, eyy, exy and
//   A1 = 2 mx my + C1, A2 = 2 (exy - mx my) + C2, B1 = mx^2 + my^2 + C1,
//   B2 = (exx - mx^2) + (eyy - my^2) + C2, S = A1 A2 / (B1 B2)
// the derivatives of S at a window position p with respect to that window's mx,
// exx and exy are
//   a = 2 my (A2 - A1) / (B1 B2) - 2 mx S / B1 + 2 mx S / B2,  b = -S / B2,  c = 2 A1 / (B1 B2)
// and every pixel q lies in the windows of the 11 x 11 positions around it, so
//   d(mean SSIM)/dx(q) = (box(a)(q) + 2 x(q) box(b)(q) + y(q) box(c)(q)) / (121 n)
// with the same zero-bordered box sum (a, b, c are 0 off the image): the
// backward is a second box pass over the maps the forward produces.
//
// paired_tile_kernel: one 256-thread block per 16 x 32 tile of one (image,
// channel) plane.
//   (1) x and y of the tile plus a halo of 10 (36 x 52) go to LDS as fp32, 0 off the image;
//   (2) 11-tap row sums of x, y, xx, yy, xy for the tile plus a halo of 5 (26 x 42
//       positions; 36 region rows), fp64, 7 consecutive outputs per thread from one
//       window held in registers (direct sum, then add the entering and subtract
//       the leaving sample);
//   (3) 11-tap column sums -> S, a, b, c per position (fp64; the tile's own
//       positions add S to the block's sum), held in registers until every
//       thread has read the row sums, then written over them;
//   (4) row sums of a, b, c (26 rows x 32 columns), (5) their column sums and the
//       gradient of the tile's own pixels, rounded to fp32 once and added to g.
// Each block writes its two fp64 partial sums (Charbonnier, SSIM) to the
// workspace; paired_fin_kernel adds them in an order that depends on the block
// count alone, so the two scalars repeat bit for bit.  All loads and stores
// are scalar fp32 accesses, whatever the alignment.
//
// Built with -ffp-contract=off: the steps round one operation at a time, as
// the float64 restatement's (tests/paired_ref.py).
#include "train_common.h"

namespace upr {

constexpr int PL_TH = UPR_PAIRED_TILE_H, PL_TW = UPR_PAIRED_TILE_W;  // tile rows (16), columns (32)
constexpr int PL_R = 5;                      // window radius
constexpr int PL_MH = PL_TH + 2 * PL_R;      // 26 rows of moment positions
constexpr int PL_MW = PL_TW + 2 * PL_R;      // 42 columns
constexpr int PL_RH = PL_MH + 2 * PL_R;      // 36 staged rows
constexpr int PL_RW = PL_MW + 2 * PL_R;      // 52 staged columns
constexpr int PL_RP = PL_RW + 1;             // padded staged row (floats)
constexpr int PL_MP = PL_MW + 1;             // padded row of moment sums (doubles)
constexpr int PL_TP = PL_TW + 1;             // padded row of a / b / c row sums
constexpr int PL_NT = 256;
constexpr int PL_RO = 7;                     // row-pass outputs per item
constexpr int PL_CO = 2;                     // column-pass outputs per item
constexpr int PL_CITEMS = (PL_MH / PL_CO) * PL_MW;             // 546
constexpr int PL_CPASS = (PL_CITEMS + PL_NT - 1) / PL_NT;      // 3
constexpr int PL_BUF = 5 * PL_RH * PL_MP;    // doubles: the five moment row sums
constexpr int PL_ABC = 3 * PL_MH * PL_MP;    // a, b, c maps; their row sums follow
static_assert(PL_MW % PL_RO == 0 && PL_MH % PL_CO == 0 && PL_TW % 4 == 0, "item maps");
static_assert(PL_TH * PL_TW == 2 * PL_NT, "two output pixels per thread");
static_assert(PL_ABC + 3 * PL_MH * PL_TP <= PL_BUF && 2 * PL_NT <= PL_BUF, "LDS reuse");

__global__ __launch_bounds__(PL_NT, 2) void paired_tile_kernel(const float* __restrict__ x,
                                                             const float* __restrict__ y, float* __restrict__ g,
                                                             double* __restrict__ part, int H, int W, int tiles_x,
                                                             int ntiles, double eps2, double c_rec, double c_ssim) {
  __shared__ float PX[PL_RH][PL_RP], PY[PL_RH][PL_RP];
  __shared__ __attribute__((aligned(16))) double buf[PL_BUF];
  double(*rows)[PL_RH][PL_MP] = (double(*)[PL_RH][PL_MP])buf;
  double(*abc)[PL_MH][PL_MP] = (double(*)[PL_MH][PL_MP])buf;
  double(*rows2)[PL_MH][PL_TP] = (double(*)[PL_MH][PL_TP])(buf + PL_ABC);
  const int t = threadIdx.x;
  const int plane = blockIdx.y, tile = blockIdx.x;
  const int ty0 = (tile / tiles_x) * PL_TH, tx0 = (tile % tiles_x) * PL_TW;
  const size_t po = (size_t)plane * H * W;
  const float* xp = x + po;
  const float* yp = y + po;

  // (1) the staged region
  for (int i = t; i < PL_RH * PL_RW; i += PL_NT) {
    const int ry = i / PL_RW, rx = i % PL_RW;
    const int gy = ty0 - 2 * PL_R + ry, gx = tx0 - 2 * PL_R + rx;
    const bool in = gy >= 0 && gy < H && gx >= 0 && gx < W;
    const int o = in ? gy * W + gx : 0;
    const float xv = xp[o], yv = yp[o];  // (element 0 exists: H, W >= 1)
    PX[ry][rx] = in ? xv : 0.f;
    PY[ry][rx] = in ? yv : 0.f;
  }
  __syncthreads();

  // (2) moment rows: item = (staged row, group of PL_RO moment columns); window = staged columns m0 .. m0 + PL_RO + 9
  for (int it = t; it < PL_RH * (PL_MW / PL_RO); it += PL_NT) {
    const int ry = it / (PL_MW / PL_RO), m0 = (it % (PL_MW / PL_RO)) * PL_RO;
    double xw[PL_RO + 10], yw[PL_RO + 10];
#pragma unroll
    for (int i = 0; i < PL_RO + 10; ++i) {
      xw[i] = (double)PX[ry][m0 + i];
      yw[i] = (double)PY[ry][m0 + i];
    }
    double s[5] = {xw[0], yw[0], xw[0] * xw[0], yw[0] * yw[0], xw[0] * yw[0]};
#pragma unroll
    for (int i = 1; i < 11; ++i) {
      s[0] += xw[i];
      s[1] += yw[i];
      s[2] += xw[i] * xw[i];
      s[3] += yw[i] * yw[i];
      s[4] += xw[i] * yw[i];
    }
#pragma unroll
    for (int q = 0; q < 5; ++q) rows[q][ry][m0] = s[q];
#pragma unroll
    for (int o = 1; o < PL_RO; ++o) {
      const double xi = xw[o + 10], yi = yw[o + 10], xo = xw[o - 1], yo = yw[o - 1];
      s[0] = (s[0] + xi) - xo;
      s[1] = (s[1] + yi) - yo;
      s[2] = (s[2] + xi * xi) - xo * xo;
      s[3] = (s[3] + yi * yi) - yo * yo;
      s[4] = (s[4] + xi * yi) - xo * yo;
#pragma unroll
      for (int q = 0; q < 5; ++q) rows[q][ry][m0 + o] = s[q];
    }
  }
  __syncthreads();

  // (3) moment columns -> S, a, b, c: item = (moment column, pair of moment rows)
  double av[PL_CPASS][PL_CO], bv[PL_CPASS][PL_CO], cv[PL_CPASS][PL_CO];
  double ssum = 0.0;
#pragma unroll
  for (int p = 0; p < PL_CPASS; ++p) {
    const int it = t + p * PL_NT;
#pragma unroll
    for (int o = 0; o < PL_CO; ++o) av[p][o] = bv[p][o] = cv[p][o] = 0.0;
    if (it < PL_CITEMS) {
      const int mx = it % PL_MW, my0 = (it / PL_MW) * PL_CO;
      double cs[5][PL_CO];
#pragma unroll
      for (int q = 0; q < 5; ++q) {
        double s = 0.0;
#pragma unroll
        for (int i = 0; i < 11; ++i) s += rows[q][my0 + i][mx];
        cs[q][0] = s;
#pragma unroll
        for (int o = 1; o < PL_CO; ++o) {
          s = (s + rows[q][my0 + o + 10][mx]) - rows[q][my0 + o - 1][mx];
          cs[q][o] = s;
        }
      }
      const int gx = tx0 - PL_R + mx;
#pragma unroll
      for (int o = 0; o < PL_CO; ++o) {
        const int my = my0 + o;
        const int gy = ty0 - PL_R + my;
        if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
          const double C1 = 0.01 * 0.01, C2 = 0.03 * 0.03;
          // two fp64 divisions per position, the rest products with the reciprocals
          const double i121 = 1.0 / 121.0;
          const double mux = cs[0][o] * i121, muy = cs[1][o] * i121;
          const double exx = cs[2][o] * i121, eyy = cs[3][o] * i121, exy = cs[4][o] * i121;
          const double mxy = mux * muy, mxx = mux * mux, myy = muy * muy;
          const double A1 = 2.0 * mxy + C1, A2 = 2.0 * (exy - mxy) + C2;
          const double B1 = (mxx + myy) + C1, B2 = ((exx - mxx) + (eyy - myy)) + C2;
          const double iB1 = 1.0 / B1, iB2 = 1.0 / B2;
          const double ibb = iB1 * iB2;
          const double S = (A1 * A2) * ibb;
          const double mS = (2.0 * mux) * S;
          av[p][o] = ((2.0 * muy) * (A2 - A1)) * ibb - mS * iB1 + mS * iB2;
          bv[p][o] = -S * iB2;
          cv[p][o] = (2.0 * A1) * ibb;
          if (my >= PL_R && my < PL_R + PL_TH && mx >= PL_R && mx < PL_R + PL_TW) ssum += S;
        }
      }
    }
  }
  __syncthreads();  // every thread has read the moment rows
#pragma unroll
  for (int p = 0; p < PL_CPASS; ++p) {
    const int it = t + p * PL_NT;
    if (it < PL_CITEMS) {
      const int mx = it % PL_MW, my0 = (it / PL_MW) * PL_CO;
#pragma unroll
      for (int o = 0; o < PL_CO; ++o) {
        abc[0][my0 + o][mx] = av[p][o];
        abc[1][my0 + o][mx] = bv[p][o];
        abc[2][my0 + o][mx] = cv[p][o];
      }
    }
  }
  __syncthreads();

  // (4) rows of a, b, c: item = (moment row, quad of tile columns); window = moment columns x0 .. x0 + 13
  for (int it = t; it < PL_MH * (PL_TW / 4); it += PL_NT) {
    const int my = it / (PL_TW / 4), x0 = (it % (PL_TW / 4)) * 4;
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      double w[14];
#pragma unroll
      for (int i = 0; i < 14; ++i) w[i] = abc[q][my][x0 + i];
      double s = w[0];
#pragma unroll
      for (int i = 1; i < 11; ++i) s += w[i];
      rows2[q][my][x0] = s;
#pragma unroll
      for (int o = 1; o < 4; ++o) {
        s = (s + w[o + 10]) - w[o - 1];
        rows2[q][my][x0 + o] = s;
      }
    }
  }
  __syncthreads();

  // (5) columns of a, b, c and the tile's own pixels: thread = (column, two tile rows)
  const int col = t % PL_TW, yb = (t / PL_TW) * 2;
  const int px = tx0 + col;
  double rsum = 0.0;
  {
    double bs[3][2];
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      double s = 0.0;
#pragma unroll
      for (int i = 0; i < 11; ++i) s += rows2[q][yb + i][col];
      bs[q][0] = s;
      bs[q][1] = (s + rows2[q][yb + 11][col]) - rows2[q][yb][col];
    }
#pragma unroll
    for (int o = 0; o < 2; ++o) {
      const int py = ty0 + yb + o;
      if (py < H && px < W) {
        const double xv = (double)PX[2 * PL_R + yb + o][2 * PL_R + col];
        const double yv = (double)PY[2 * PL_R + yb + o][2 * PL_R + col];
        const double d = xv - yv;
        const double r = sqrt(d * d + eps2);
        rsum += r;
        if (g) {
          const double ds = (bs[0][o] + (2.0 * xv) * bs[1][o]) + yv * bs[2][o];
          const double gr = c_rec * (d / r) - c_ssim * ds;
          float* gp = g + po + (size_t)py * W + px;
          *gp = *gp + (float)gr;
        }
      }
    }
  }

  // the block's two sums in a fixed order
  __syncthreads();  // the last pass has read the a / b / c row sums
  buf[t] = rsum;
  buf[PL_NT + t] = ssum;
  __syncthreads();
  for (int s = PL_NT / 2; s > 0; s >>= 1) {
    if (t < s) {
      buf[t] += buf[t + s];
      buf[PL_NT + t] += buf[PL_NT + t + s];
    }
    __syncthreads();
  }
  if (t < 2) part[((size_t)plane * ntiles + tile) * 2 + t] = buf[t * PL_NT];
}

// one block: thread t adds partials t, t + 256, ..., then a fixed tree
__global__ __launch_bounds__(256) void paired_fin_kernel(const double* __restrict__ part, long long nparts, double n,
                                                         float w_rec, float w_ssim, float* __restrict__ out2,
                                                         float* __restrict__ total) {
  __shared__ double red[2][256];
  const int t = threadIdx.x;
  double a = 0.0, b = 0.0;
  for (long long i = t; i < nparts; i += 256) {
    a += part[2 * i];
    b += part[2 * i + 1];
  }
  red[0][t] = a;
  red[1][t] = b;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (t < s) {
      red[0][t] += red[0][t + s];
      red[1][t] += red[1][t + s];
    }
    __syncthreads();
  }
  if (t == 0) {
    const float rec = (float)(red[0][0] / n);
    const float sl = (float)(1.0 - red[1][0] / n);
    out2[0] = rec;
    out2[1] = sl;
    if (total) *total = *total + (w_rec * rec + w_ssim * sl);
  }
}

static inline long long paired_tiles(int H, int W) { return (long long)cdiv(H, PL_TH) * cdiv(W, PL_TW); }

// a plane is indexed with ints, the tile count rides on blockIdx.x
static bool paired_shape_ok(int B, int H, int W) {
  return B >= 1 && H >= 1 && W >= 1 && (long long)H * W < (1LL << 31) && paired_tiles(H, W) < (1LL << 31);
}

}  // namespace upr

using namespace upr;

extern "C" {

size_t upr_t_loss_paired_workspace(int B, int H, int W) {
  if (!paired_shape_ok(B, H, W)) return 0;
  return (size_t)B * 3 * (size_t)paired_tiles(H, W) * 2 * sizeof(double);
}

int upr_t_loss_paired(const float* enh, const float* target, int B, int H, int W, float eps, float w_rec, float w_ssim,
                      void* ws, size_t ws_bytes, float* out2, float* total, float* g_enh, void* stream) {
  if (B == 0) return UPR_OK;
  if (!enh || !target || !out2 || !ws) return UPR_ERR_ARG;
  if (!paired_shape_ok(B, H, W)) return UPR_ERR_SHAPE;
  if ((uintptr_t)ws % 8) return UPR_ERR_ARG;
  if (ws_bytes < upr_t_loss_paired_workspace(B, H, W)) return UPR_ERR_WORKSPACE;
  const int tiles_x = cdiv(W, PL_TW), ntiles = (int)paired_tiles(H, W);
  const long long planes = (long long)B * 3;
  const double n = (double)planes * (double)H * (double)W;
  double* part = (double*)ws;
  // (blockIdx.y carries the plane: at most 65535 per launch)
  for (long long p0 = 0; p0 < planes; p0 += 65535) {
    const int np = (int)(planes - p0 < 65535 ? planes - p0 : 65535);
    const size_t io = (size_t)p0 * H * W;
    hipLaunchKernelGGL(paired_tile_kernel, dim3(ntiles, np), dim3(PL_NT), 0, ST(stream), enh + io, target + io,
                       g_enh ? g_enh + io : nullptr, part + (size_t)p0 * ntiles * 2, H, W, tiles_x, ntiles,
                       (double)eps * (double)eps, (double)w_rec / n, (double)w_ssim / (121.0 * n));
    const int rc = (int)hipGetLastError();
    if (rc) return rc;
  }
  hipLaunchKernelGGL(paired_fin_kernel, dim3(1), dim3(256), 0, ST(stream), (const double*)part, planes * ntiles, n,
                     w_rec, w_ssim, out2, total);
  LAUNCH_CHECK();
}

}  // extern "C"
