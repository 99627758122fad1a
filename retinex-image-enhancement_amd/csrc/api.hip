// C ABI of the enhancer kernels (see include/upr.h for the contract of each).
#include <cstring>

#include "upr_common.h"
#include "lab_tables.h"
#include "../../include/upr.h"

namespace upr {
int launch_clahe_pipeline(const void* enh, void* out, uint8_t* ws, int B, int H, int W, float clip, int tilesX,
                          int tilesY, int dtype, hipStream_t st);
size_t clahe_pipeline_ws(int B, int H, int W, int tilesX, int tilesY);
int launch_clahe_u8(const uint8_t* src, uint8_t* dst, uint8_t* lut, int B, int H, int W, float clip, int tilesX,
                    int tilesY, hipStream_t st);
int launch_rgb2lab(const uint8_t* rgb, uint8_t* lab, size_t npix, hipStream_t st);
int launch_lab2rgb(const uint8_t* lab, uint8_t* rgb, size_t npix, hipStream_t st);
int launch_quantize(const void* x, uint8_t* out, size_t n, int dtype, hipStream_t st);
int launch_to_u8_hwc(const void* x, int C, int H, int W, int dtype, uint8_t* out, hipStream_t st);
int launch_letterbox(const void* src, int src_kind, int H, int W, int top, int left, int nh, int nw, int Ho, int Wo,
                     const int* xtab, const int* ytab, int color, void* out, int out_kind, hipStream_t st);
int launch_letterbox_batch(const upr_letterbox_rec* recs, int B, int Ho, int Wo, int color, void* out, int dtype,
                           hipStream_t st);
int launch_panels_u8(const void* x, const void* enh, const void* illu, int B, int H, int W, int dtype, uint8_t* enh_u8,
                     uint8_t* illu_u8, uint8_t* cmp_u8, int P, hipStream_t st);
int launch_gray_hist(const void* img, int* hist, int B, int H, int W, int dtype, hipStream_t st);
int launch_multiscale(const void* x, const void* enh, void* out, double* sums, double* factor, int B, int H, int W,
                      int dtype, hipStream_t st);
int launch_ms_features(const void* x, void* out, int B, int H, int W, int scale_idx, int dtype, hipStream_t st);
size_t content_aware_ws(int B, int H, int W);
int launch_content_aware(const void* x, const void* enh, void* out, float* sal_out, float* att_out, uint8_t* ws,
                         int B, int H, int W, int dtype, hipStream_t st);
size_t metrics_ws(int B, int H, int W);
int launch_metrics(const void* enh, const void* ref, double* metrics, double* sums, int* hist, uint8_t* ws, int B,
                   int H, int W, int dtype, hipStream_t st);
size_t loe_ws(int B);
int launch_loe(const void* low, const void* enh, double* loe, long long* counts, uint8_t* ws, int B, int H, int W,
               int sample, int dtype, hipStream_t st);
int launch_decompose(const void* x, const void* illu, void* refl, int B, int C, int HW, int illu_c, int dtype,
                     hipStream_t st);
int launch_decompose_bwd(const void* x, const void* illu, const void* g, void* gx, void* gillu, int B, int C, int HW,
                         int illu_c, int dtype, hipStream_t st);
int png_bound(int H, int W, int rows_per_strip, int match, size_t* bytes_per_image, size_t* scratch_bytes);
int launch_png_encode(const uint8_t* img, int B, int H, int W, int filter, int match, int rows_per_strip, uint8_t* out,
                      size_t out_stride, long long* sizes, uint8_t* scratch, size_t scratch_bytes, hipStream_t st);
int jpeg_bound(int H, int W, int restart_rows, int subsampling, int huffman, size_t* bytes_per_image,
               size_t* scratch_bytes);
int launch_jpeg_encode(const uint8_t* img, int B, int H, int W, int quality, int restart_rows, int subsampling,
                       int huffman, uint8_t* out, size_t out_stride, long long* sizes, uint8_t* scratch,
                       size_t scratch_bytes, hipStream_t st);
int launch_jpeg_huffman_build(const uint32_t* freq, int n, uint8_t* bits_vals, int32_t* nvals, hipStream_t st);
}  // namespace upr

using namespace upr;

static bool dtype_ok(int dt) { return dt == UPR_F32 || dt == UPR_F16; }

extern "C" {

int upr_quantize_u8(const void* x, uint8_t* out, size_t n, int dtype, void* stream) {
  if (!x || !out || !dtype_ok(dtype)) return UPR_ERR_ARG;
  if (n == 0) return UPR_OK;
  return launch_quantize(x, out, n, dtype, (hipStream_t)stream);
}

int upr_letterbox(const void* src, int src_kind, int H, int W, int top, int left, int nh, int nw, int Ho, int Wo,
                  const int32_t* xtab, const int32_t* ytab, int color, void* out, int out_kind, void* stream) {
  if (!src || !out || (src_kind != 0 && src_kind != 1) || (out_kind != 0 && out_kind != 1)) return UPR_ERR_ARG;
  if (H <= 0 || W <= 0 || nh <= 0 || nw <= 0 || top < 0 || left < 0 || top + nh > Ho || left + nw > Wo)
    return UPR_ERR_SHAPE;
  if ((xtab == nullptr) != (ytab == nullptr)) return UPR_ERR_ARG;
  if (!xtab && (nh != H || nw != W)) return UPR_ERR_SHAPE;
  return launch_letterbox(src, src_kind, H, W, top, left, nh, nw, Ho, Wo, xtab, ytab, color, out, out_kind,
                          (hipStream_t)stream);
}

int upr_to_u8_hwc(const void* x, int C, int H, int W, int dtype, uint8_t* out, void* stream) {
  if (!x || !out || !dtype_ok(dtype) || (C != 1 && C != 3)) return UPR_ERR_ARG;
  if (H <= 0 || W <= 0) return UPR_ERR_SHAPE;
  return launch_to_u8_hwc(x, C, H, W, dtype, out, (hipStream_t)stream);
}

int upr_letterbox_batch(const upr_letterbox_rec* rec_dev, int B, int Ho, int Wo, int color, void* out, int dtype,
                        void* stream) {
  if (!rec_dev || !out || B < 1 || !dtype_ok(dtype)) return UPR_ERR_ARG;
  if (Ho <= 0 || Wo <= 0 || B > 65535) return UPR_ERR_SHAPE;
  return launch_letterbox_batch(rec_dev, B, Ho, Wo, color, out, dtype, (hipStream_t)stream);
}

int upr_panels_u8(const void* x, const void* enh, const void* illu, int B, int H, int W, int dtype, uint8_t* enh_u8,
                  uint8_t* illu_u8, uint8_t* cmp_u8, int cmp_panels, void* stream) {
  if (!x || !enh || !enh_u8 || B < 1 || !dtype_ok(dtype)) return UPR_ERR_ARG;
  if (illu_u8 && !illu) return UPR_ERR_ARG;
  if (cmp_u8 && ((cmp_panels != 2 && cmp_panels != 3) || (cmp_panels == 3 && !illu))) return UPR_ERR_ARG;
  if (H <= 0 || W <= 0 || B > 65535) return UPR_ERR_SHAPE;
  return launch_panels_u8(x, enh, illu, B, H, W, dtype, enh_u8, illu_u8, cmp_u8, cmp_panels, (hipStream_t)stream);
}

int upr_rgb2lab_u8(const uint8_t* rgb, uint8_t* lab, size_t npix, void* stream) {
  if (!rgb || !lab) return UPR_ERR_ARG;
  if (npix == 0) return UPR_OK;
  return launch_rgb2lab(rgb, lab, npix, (hipStream_t)stream);
}

int upr_lab2rgb_u8(const uint8_t* lab, uint8_t* rgb, size_t npix, void* stream) {
  if (!rgb || !lab) return UPR_ERR_ARG;
  if (npix == 0) return UPR_OK;
  return launch_lab2rgb(lab, rgb, npix, (hipStream_t)stream);
}

int upr_clahe_u8(const uint8_t* src, uint8_t* dst, uint8_t* lut_ws, int B, int H, int W, float clip, int tiles_x,
                 int tiles_y, void* stream) {
  if (!src || !dst || !lut_ws || B <= 0 || H <= 0 || W <= 0 || tiles_x <= 0 || tiles_y <= 0) return UPR_ERR_ARG;
  if (tiles_x > W || tiles_y > H) return UPR_ERR_SHAPE;
  return launch_clahe_u8(src, dst, lut_ws, B, H, W, clip, tiles_x, tiles_y, (hipStream_t)stream);
}

size_t upr_clahe_enhance_workspace(int B, int H, int W, int tiles_x, int tiles_y) {
  if (B <= 0 || H <= 0 || W <= 0 || tiles_x <= 0 || tiles_y <= 0) return 0;
  return clahe_pipeline_ws(B, H, W, tiles_x, tiles_y);
}

int upr_clahe_enhance(const void* enh, void* out, void* workspace, int B, int H, int W, float clip, int tiles_x,
                      int tiles_y, int dtype, void* stream) {
  if (!enh || !out || !workspace || B <= 0 || H <= 0 || W <= 0 || !dtype_ok(dtype)) return UPR_ERR_ARG;
  if (tiles_x <= 0 || tiles_y <= 0 || tiles_x > W || tiles_y > H) return UPR_ERR_SHAPE;
  return launch_clahe_pipeline(enh, out, (uint8_t*)workspace, B, H, W, clip, tiles_x, tiles_y, dtype,
                               (hipStream_t)stream);
}

int upr_gray_hist(const void* x, int32_t* hist, int B, int H, int W, int dtype, void* stream) {
  if (!x || !hist || B <= 0 || H <= 0 || W <= 0 || !dtype_ok(dtype)) return UPR_ERR_ARG;
  return launch_gray_hist(x, hist, B, H, W, dtype, (hipStream_t)stream);
}

int upr_multiscale(const void* x, const void* enh, void* out, double* sums, double* factor, int B, int H, int W,
                   int dtype, void* stream) {
  if (!x || !sums || B <= 0 || H <= 0 || W <= 0 || !dtype_ok(dtype)) return UPR_ERR_ARG;
  if (H < 8 || W < 8) return UPR_ERR_SHAPE;  // torch.gradient needs >= 2 samples at the 1/4 scale
  return launch_multiscale(x, enh, out, sums, factor, B, H, W, dtype, (hipStream_t)stream);
}

int upr_multiscale_features(const void* x, void* out, int B, int H, int W, int scale_idx, int dtype, void* stream) {
  if (!x || !out || B <= 0 || H <= 0 || W <= 0 || scale_idx < 0 || scale_idx > 2 || !dtype_ok(dtype))
    return UPR_ERR_ARG;
  return launch_ms_features(x, out, B, H, W, scale_idx, dtype, (hipStream_t)stream);
}

size_t upr_content_aware_workspace(int B, int H, int W) {
  if (B <= 0 || H <= 0 || W <= 0) return 0;
  return content_aware_ws(B, H, W);
}

int upr_content_aware(const void* x, const void* enh, void* out, float* saliency, float* attention, void* workspace,
                      size_t workspace_bytes, int B, int H, int W, int dtype, void* stream) {
  if (!x || !workspace || B <= 0 || H <= 0 || W <= 0 || !dtype_ok(dtype)) return UPR_ERR_ARG;
  if ((enh == nullptr) != (out == nullptr)) return UPR_ERR_ARG;
  if (workspace_bytes < content_aware_ws(B, H, W)) return UPR_ERR_WORKSPACE;
  return launch_content_aware(x, enh, out, saliency, attention, (uint8_t*)workspace, B, H, W, dtype,
                              (hipStream_t)stream);
}

size_t upr_image_metrics_workspace(int B, int H, int W) {
  if (B <= 0 || H <= 0 || W <= 0) return 0;
  return metrics_ws(B, H, W);
}

int upr_image_metrics(const void* enh, const void* ref, double* metrics, double* sums, int32_t* hist,
                      void* workspace, size_t workspace_bytes, int B, int H, int W, int dtype, void* stream) {
  if (!enh || !metrics || !workspace || !dtype_ok(dtype)) return UPR_ERR_ARG;
  // (one image's byte offsets are 32-bit buffer offsets, and 2^30 must lie past the image)
  if (B < 1 || H < 8 || W < 8 || (long long)H * W * 3 * 4 > 0x40000000LL) return UPR_ERR_SHAPE;
  if (workspace_bytes < metrics_ws(B, H, W)) return UPR_ERR_WORKSPACE;
  return launch_metrics(enh, ref, metrics, sums, hist, (uint8_t*)workspace, B, H, W, dtype, (hipStream_t)stream);
}

size_t upr_image_loe_workspace(int B) { return B > 0 ? loe_ws(B) : 0; }

int upr_image_loe(const void* low, const void* enh, double* loe, int64_t* counts, void* workspace,
                  size_t workspace_bytes, int B, int H, int W, int sample, int dtype, void* stream) {
  if (!low || !enh || !loe || !workspace || !dtype_ok(dtype) || sample < 0) return UPR_ERR_ARG;
  // (grid pixel indices and the table's entries are int32)
  if (B < 1 || H < 1 || W < 1 || (long long)H * W >= (1LL << 31)) return UPR_ERR_SHAPE;
  if (workspace_bytes < loe_ws(B)) return UPR_ERR_WORKSPACE;
  return launch_loe(low, enh, loe, (long long*)counts, (uint8_t*)workspace, B, H, W, sample, dtype,
                    (hipStream_t)stream);
}

int upr_retinex_decompose(const void* x, const void* illu, void* refl, int B, int C, int H, int W, int illu_c,
                          int dtype, void* stream) {
  if (!x || !illu || !refl || !dtype_ok(dtype) || B <= 0 || C <= 0 || (illu_c != 1 && illu_c != C)) return UPR_ERR_ARG;
  if (H <= 0 || W <= 0 || (long long)B * H * W * C >= (1LL << 40)) return UPR_ERR_SHAPE;
  return launch_decompose(x, illu, refl, B, C, H * W, illu_c, dtype, (hipStream_t)stream);
}

int upr_retinex_decompose_bwd(const void* x, const void* illu, const void* g, void* gx, void* gillu, int B, int C,
                              int H, int W, int illu_c, int dtype, void* stream) {
  if (!x || !illu || !g || !dtype_ok(dtype) || B <= 0 || C <= 0 || (illu_c != 1 && illu_c != C)) return UPR_ERR_ARG;
  if (H <= 0 || W <= 0) return UPR_ERR_SHAPE;
  if (!gx && !gillu) return UPR_OK;
  return launch_decompose_bwd(x, illu, g, gx, gillu, B, C, H * W, illu_c, dtype, (hipStream_t)stream);
}

int upr_png_bound_ex(int H, int W, int rows_per_strip, int match, size_t* bytes_per_image, size_t* scratch_bytes) {
  if (!bytes_per_image || !scratch_bytes) return UPR_ERR_ARG;
  if (match != UPR_PNG_MATCH_NONE && match != UPR_PNG_MATCH_LZ) return UPR_ERR_ARG;
  return png_bound(H, W, rows_per_strip, match, bytes_per_image, scratch_bytes);
}

int upr_png_bound(int H, int W, int rows_per_strip, size_t* bytes_per_image, size_t* scratch_bytes) {
  return upr_png_bound_ex(H, W, rows_per_strip, UPR_PNG_MATCH_NONE, bytes_per_image, scratch_bytes);
}

int upr_png_encode_ex(const uint8_t* hwc_u8, int B, int H, int W, int filter, int match, int rows_per_strip,
                      uint8_t* out, size_t out_stride, int64_t* sizes, void* scratch, size_t scratch_bytes,
                      void* stream) {
  if (!hwc_u8 || !out || !sizes || !scratch || B <= 0 || H <= 0 || W <= 0 || rows_per_strip <= 0) return UPR_ERR_ARG;
  if (filter < UPR_PNG_FILTER_NONE || filter > UPR_PNG_FILTER_ADAPTIVE || ((size_t)scratch & 15)) return UPR_ERR_ARG;
  if (match != UPR_PNG_MATCH_NONE && match != UPR_PNG_MATCH_LZ) return UPR_ERR_ARG;
  return launch_png_encode(hwc_u8, B, H, W, filter, match, rows_per_strip, out, out_stride, (long long*)sizes,
                           (uint8_t*)scratch, scratch_bytes, (hipStream_t)stream);
}

int upr_png_encode(const uint8_t* hwc_u8, int B, int H, int W, int filter, int rows_per_strip, uint8_t* out,
                   size_t out_stride, int64_t* sizes, void* scratch, size_t scratch_bytes, void* stream) {
  return upr_png_encode_ex(hwc_u8, B, H, W, filter, UPR_PNG_MATCH_NONE, rows_per_strip, out, out_stride, sizes, scratch,
                           scratch_bytes, stream);
}

static bool jpeg_modes_ok(int subsampling, int huffman) {
  return subsampling >= UPR_JPEG_444 && subsampling <= UPR_JPEG_GRAY &&
         (huffman == UPR_JPEG_HUFF_STANDARD || huffman == UPR_JPEG_HUFF_OPTIMIZED);
}

int upr_jpeg_bound_ex(int H, int W, int restart_rows, int subsampling, int huffman, size_t* bytes_per_image,
                      size_t* scratch_bytes) {
  if (!bytes_per_image || !scratch_bytes || !jpeg_modes_ok(subsampling, huffman)) return UPR_ERR_ARG;
  return jpeg_bound(H, W, restart_rows, subsampling, huffman, bytes_per_image, scratch_bytes);
}

int upr_jpeg_bound(int H, int W, int restart_rows, size_t* bytes_per_image, size_t* scratch_bytes) {
  return upr_jpeg_bound_ex(H, W, restart_rows, UPR_JPEG_444, UPR_JPEG_HUFF_STANDARD, bytes_per_image, scratch_bytes);
}

int upr_jpeg_encode_ex(const uint8_t* hwc_u8, int B, int H, int W, int quality, int restart_rows, int subsampling,
                       int huffman, uint8_t* out, size_t out_stride, int64_t* sizes, void* scratch,
                       size_t scratch_bytes, void* stream) {
  if (!hwc_u8 || !out || !sizes || !scratch || B <= 0 || H <= 0 || W <= 0 || restart_rows <= 0) return UPR_ERR_ARG;
  if (quality < 1 || quality > 100 || ((size_t)scratch & 15) || !jpeg_modes_ok(subsampling, huffman))
    return UPR_ERR_ARG;
  return launch_jpeg_encode(hwc_u8, B, H, W, quality, restart_rows, subsampling, huffman, out, out_stride,
                            (long long*)sizes, (uint8_t*)scratch, scratch_bytes, (hipStream_t)stream);
}

int upr_jpeg_encode(const uint8_t* hwc_u8, int B, int H, int W, int quality, int restart_rows, uint8_t* out,
                    size_t out_stride, int64_t* sizes, void* scratch, size_t scratch_bytes, void* stream) {
  return upr_jpeg_encode_ex(hwc_u8, B, H, W, quality, restart_rows, UPR_JPEG_444, UPR_JPEG_HUFF_STANDARD, out,
                            out_stride, sizes, scratch, scratch_bytes, stream);
}

int upr_jpeg_huffman_build(const uint32_t* freq, int n, uint8_t* bits_vals, int32_t* nvals, void* stream) {
  if (!freq || !bits_vals || !nvals || n <= 0) return UPR_ERR_ARG;
  return launch_jpeg_huffman_build(freq, n, bits_vals, nvals, (hipStream_t)stream);
}

void upr_lab_tables(uint16_t* gamma, uint16_t* cbrt, uint16_t* yf, uint16_t* invgamma, int32_t* rgb2xyz,
                    int32_t* xyz2rgb) {
  const LabTables& t = lab_tables();
  if (gamma) memcpy(gamma, t.gamma_b, sizeof(t.gamma_b));
  if (cbrt) memcpy(cbrt, t.cbrt_b, sizeof(t.cbrt_b));
  if (yf) memcpy(yf, t.yf_b, sizeof(t.yf_b));
  if (invgamma) memcpy(invgamma, t.invgamma_b, sizeof(t.invgamma_b));
  if (rgb2xyz) memcpy(rgb2xyz, t.rgb2xyz, sizeof(t.rgb2xyz));
  if (xyz2rgb) memcpy(xyz2rgb, t.xyz2rgb, sizeof(t.xyz2rgb));
}

}  // extern "C"
