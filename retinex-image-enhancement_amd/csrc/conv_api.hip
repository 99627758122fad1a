// Op-level C entry points of the inference convs and of the split forms
// (include/upr.h): one conv per call on whole NHWC tensors, the two weight
// packers, the fp32 <-> split-fp16 tensor passes.  The switches of the split
// forms are read at every call here (read_split_switches).
#include <cstring>

#include "split_pack.h"
#include "../../include/upr.h"

using namespace upr;

// The checks the conv entry points share -- pointers and sizes (UPR_ERR_ARG),
// then an output of at least one pixel (UPR_ERR_SHAPE) -- and the op they all
// start from: one plain NHWC segment, Kpad = kh kw Cin, bias, ReLU, y as a
// whole NHWC tensor.  The residual, channel multiples and form are the caller's.
static int conv_op_nhwc(ConvOp& c, const void* x, int B, int H, int W, int Cin, const void* w, const float* bias,
                        int Cout, int kh, int kw, int stride, int pad, int dil, int relu, void* y) {
  if (!x || !w || !y || B <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0) return UPR_ERR_ARG;
  if (kh <= 0 || kw <= 0 || stride <= 0 || dil <= 0 || pad < 0) return UPR_ERR_ARG;
  const int Ho = (H + 2 * pad - dil * (kh - 1) - 1) / stride + 1;
  const int Wo = (W + 2 * pad - dil * (kw - 1) - 1) / stride + 1;
  if (Ho <= 0 || Wo <= 0) return UPR_ERR_SHAPE;
  memset(&c, 0, sizeof(c));
  c.nseg = 1;
  ConvSeg& s = c.seg[0];
  s.src = x; s.C = Cin; s.cs = Cin; s.coff = 0; s.Hin = H; s.Win = W;
  s.kh = kh; s.kw = kw; s.stride = stride; s.pad = pad; s.dil = dil; s.pre = kPreNone; s.kbase = 0;
  c.B = B; c.Ho = Ho; c.Wo = Wo; c.N = Cout; c.Kpad = kh * kw * Cin;
  c.W = w; c.bias = bias; c.relu = relu;
  c.out = y; c.out_cs = Cout; c.out_coff = 0; c.store = kStoreNHWC;
  return UPR_OK;
}

extern "C" {

int upr_conv2d_nhwc(const void* x, int B, int H, int W, int Cin, const void* w, const float* bias, int Cout, int kh,
                    int kw, int stride, int pad, int dil, const void* residual, int relu, void* y, int dtype,
                    void* stream) {
  if (dtype == UPR_F32_SPLIT_REGS)
    return upr_conv2d_nhwc_regs(x, B, H, W, Cin, w, bias, Cout, kh, kw, stride, pad, dil, residual, relu, y, nullptr,
                                stream);
  if (Cin % 32 || Cout % 32 || (dtype != UPR_F32 && dtype != UPR_F16 && dtype != UPR_F32_SPLIT)) return UPR_ERR_ARG;
  ConvOp c;
  const int rc = conv_op_nhwc(c, x, B, H, W, Cin, w, bias, Cout, kh, kw, stride, pad, dil, relu, y);
  if (rc != UPR_OK) return rc;
  // without ReLU, "added before" and "added after" coincide: use the post-ReLU
  // slot, which every kernel family takes
  if (relu) { c.res1 = residual; c.res1_cs = Cout; }
  else { c.res2 = residual; c.res2_cs = Cout; }
  if (dtype != UPR_F32_SPLIT) return launch_conv(c, dtype, (hipStream_t)stream);
  // x / residual / y are split tensors, w is upr_pack_split_f32's blob: the
  // two K-segments of pack_split over x, then the per-channel scale
  if (Cin % 64 || Cout % 128) return UPR_ERR_UNSUPPORTED;
  const int taps = kh * kw;
  c.nseg = 2;
  c.seg[0].C = 2 * Cin; c.seg[0].cs = 2 * Cin;
  c.seg[1] = c.seg[0];
  c.seg[1].C = Cin; c.seg[1].kbase = taps * 2 * Cin;
  c.Kpad = (int)align_up((size_t)3 * taps * Cin, 32);
  c.scale = (const float*)((const uint8_t*)w + align_up((size_t)Cout * c.Kpad * 2, 256));
  c.res1_cs *= 2; c.res2_cs *= 2;
  c.split_res = residual != nullptr;
  c.out = nullptr; c.out_cs = 0;
  c.split_out = y; c.split_cs = 2 * Cout; c.split_lo = Cout;
  return launch_conv_wide(c, (hipStream_t)stream);
}

int upr_conv2d_nhwc_regs(const void* x, int B, int H, int W, int Cin, const void* w, const float* bias, int Cout,
                         int kh, int kw, int stride, int pad, int dil, const void* residual, int relu, void* y,
                         unsigned* overflow, void* stream) {
  if (Cin % 32 || Cout % 32) return UPR_ERR_ARG;
  // the UPR_F32 op of upr_conv2d_nhwc, offered in the split-in-registers form to
  // the kernels that have it and to nothing else
  ConvOp c;
  const int rc = conv_op_nhwc(c, x, B, H, W, Cin, w, bias, Cout, kh, kw, stride, pad, dil, relu, y);
  if (rc != UPR_OK) return rc;
  // (the row ring adds its residual after the ReLU; with a ReLU its pre-ReLU
  // residual program is the dilation-2 FAM part, which this entry does not offer)
  if (relu && residual) return UPR_ERR_UNSUPPORTED;
  c.res2 = residual; c.res2_cs = Cout;
  c.mma16 = kMma16Offer; c.ovf = overflow;
  c.ring_split = read_split_switches().ring_split;  // read at the call: one process can run both programs
  return launch_conv_regs(c, (hipStream_t)stream);
}

size_t upr_pack_split_f32(const float* w, int Cout, int Cin, int kh, int kw, void* out, size_t out_bytes) {
  if (!w || Cout <= 0 || Cin <= 0 || Cin % 64 || kh <= 0 || kw <= 0) return 0;
  std::vector<SegWeights> segs(1);
  segs[0].spec = seg(/*src=*/0, Cin, Cin, 0, kh, 1, 0, 1);
  segs[0].spec.kw = kw;
  segs[0].w.assign(w, w + (size_t)Cout * Cin * kh * kw);
  SplitPack sp;
  if (!pack_split(Cout, segs, sp)) return 0;
  const size_t wbytes = align_up(sp.W.size() * 2, 256), need = wbytes + sp.scale.size() * 4;
  if (out && out_bytes >= need) {
    memset(out, 0, need);
    memcpy(out, sp.W.data(), sp.W.size() * 2);
    memcpy((uint8_t*)out + wbytes, sp.scale.data(), sp.scale.size() * 4);
  }
  return need;
}

size_t upr_pack_split_w_f32(const float* w, int Cout, int Cin, int kh, int kw, const float* w2, int C2, void* out,
                            size_t out_bytes) {
  if (!w || Cout <= 0 || Cout % 64 || Cin <= 0 || Cin % 32 || kh <= 0 || kw <= 0) return 0;
  if ((w2 != nullptr) != (C2 > 0) || C2 < 0 || C2 % 32) return 0;
  const int K1 = kh * kw * Cin, K = K1 + C2;
  std::vector<float> rows((size_t)Cout * K);
  for (int n = 0; n < Cout; ++n) {
    memcpy(rows.data() + (size_t)n * K, w + (size_t)n * K1, (size_t)K1 * 4);
    if (w2) memcpy(rows.data() + (size_t)n * K + K1, w2 + (size_t)n * C2, (size_t)C2 * 4);
  }
  SplitWPack sp;
  if (!pack_split_w(Cout, K, rows.data(), sp)) return 0;
  size_t soff = 0;
  const size_t need = split_w_bytes(Cout, K, &soff);
  if (out && out_bytes >= need) {
    memset(out, 0, need);
    memcpy(out, sp.W.data(), sp.W.size() * 2);
    memcpy((uint8_t*)out + soff, sp.scale.data(), sp.scale.size() * 4);
  }
  return need;
}

// the kernel the calling thread's latest upr_conv2d_nhwc_wsplit ran
// (kWSplitNone when it refused the op, at whichever check)
static thread_local int t_wsplit_ran = kWSplitNone;

int upr_conv2d_nhwc_wsplit(const void* x, int B, int H, int W, int Cin, const void* blob, size_t blob_bytes,
                           const float* bias, int Cout, int kh, int kw, int stride, int pad, int dil,
                           const void* residual, int relu, void* y, const void* x2, int H2, int W2, int C2,
                           int stride2, unsigned* overflow, void* stream) {
  t_wsplit_ran = kWSplitNone;
  if (x2 && (H2 <= 0 || W2 <= 0 || C2 <= 0 || stride2 <= 0)) return UPR_ERR_ARG;
  ConvOp c;
  const int rc = conv_op_nhwc(c, x, B, H, W, Cin, blob, bias, Cout, kh, kw, stride, pad, dil, relu, y);
  if (rc != UPR_OK) return rc;
  if (x2 && ((H2 - 1) / stride2 + 1 != c.Ho || (W2 - 1) / stride2 + 1 != c.Wo)) return UPR_ERR_SHAPE;
  if (Cin % 32 || Cout % 64 || (x2 && C2 % 32)) return UPR_ERR_UNSUPPORTED;
  const int K1 = c.Kpad, K = K1 + (x2 ? C2 : 0);
  size_t soff = 0;
  if (blob_bytes != split_w_bytes(Cout, K, &soff)) return UPR_ERR_UNSUPPORTED;  // packed for another shape
  if (x2) {
    c.nseg = 2;
    ConvSeg& t = c.seg[1];
    t.src = x2; t.C = C2; t.cs = C2; t.coff = 0; t.Hin = H2; t.Win = W2;
    t.kh = 1; t.kw = 1; t.stride = stride2; t.pad = 0; t.dil = 1; t.pre = kPreNone; t.kbase = K1;
  }
  c.Kpad = K;
  c.scale = (const float*)((const uint8_t*)blob + soff);
  c.res2 = residual; c.res2_cs = Cout;
  c.mma16 = kMma16WSplit; c.ovf = overflow;
  // read at the call: one process can run both kernels and both ring schedules
  const SplitSwitches sw = read_split_switches();
  c.ring_split = sw.ring_split;
  c.w64_tile = sw.w64_tile;
  return launch_conv_wsplit(c, (hipStream_t)stream, &t_wsplit_ran);
}

int upr_conv_wsplit_ran(void) { return t_wsplit_ran; }

int upr_split_f32(const float* x, void* y, size_t npix, int C, unsigned* overflow, void* stream) {
  if (!x || !y) return UPR_ERR_ARG;
  return launch_split_f32(x, y, npix, C, overflow, (hipStream_t)stream);
}

int upr_unsplit_f32(const void* x, float* y, size_t npix, int C, void* stream) {
  if (!x || !y) return UPR_ERR_ARG;
  return launch_unsplit_f32(x, y, npix, C, (hipStream_t)stream);
}

}  // extern "C"
