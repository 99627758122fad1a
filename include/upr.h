/*
 * upr.h — C ABI of libupr.so, the MI355X (gfx950) UP-Retinex kernel library.
 *
 * The reference (xh92117/Retinex-image-Enhancement) has no native code and no
 * FFI: its hot path is the Python/PyTorch surface below.  Each entry point
 * names the reference interface it replaces (file:line, relative to the
 * reference root).  Conventions:
 *   - every buffer is caller-allocated device memory unless stated otherwise
 *     (params of upr_model_create are HOST fp32 arrays); the library never
 *     frees caller memory;
 *   - `stream` is a hipStream_t passed as void*; launches are stream-ordered
 *     and never synchronise internally;
 *   - images are NCHW with C = 3 (the reference's tensor layout), dtype
 *     UPR_F32 (float) or UPR_F16 (IEEE half);
 *   - return 0 on success, a hipError_t value (> 0) passed through, or a
 *     negative UPR_ERR_* code; upr_status_string() describes either.
 * Thread safety: distinct models / streams may be used concurrently; one model
 * handle must not be used on two streams at once.  A forward (fp32 or fp16;
 * UPR_MS_STREAMS=0 turns it off) forks its multi-scale head onto a side stream
 * of the library's own, keyed by (device, caller stream), with fork / join
 * events of that side.  NULL is treated as the one legacy stream: it forks
 * too, and two threads forwarding on NULL share one side stream and its
 * events, so a handle -- or two handles -- must not be used from two threads
 * on NULL at once.  hipStreamPerThread (a different real stream per thread)
 * never forks: such forwards run on the one stream.
 */
#ifndef UPR_H_
#define UPR_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* upr_conv2d_nhwc only: UPR_F32_SPLIT -- an fp32 conv computed from split-fp16
 * operands (see upr_split_f32); UPR_F32_SPLIT_REGS -- an fp32 conv over plain
 * fp32 tensors whose fragments are split into fp16 (hi, lo) pairs in registers
 * (see upr_conv2d_nhwc_regs) */
enum { UPR_F32 = 0, UPR_F16 = 1, UPR_F32_SPLIT = 2, UPR_F32_SPLIT_REGS = 3 };

enum {
  UPR_OK = 0,
  UPR_ERR_ARG = -1,
  UPR_ERR_SHAPE = -2,
  UPR_ERR_MISSING_PARAM = -3,
  UPR_ERR_WORKSPACE = -4,
  UPR_ERR_UNSUPPORTED = -5
};

/* model flags: UPR_MODEL_IENET_ONLY = ResidualIENet alone; UPR_MODEL_HEAD_ONLY =
 * MultiScaleUP_Retinex.multi_scale_enhance alone (the 3-scale FAM head, the
 * enhancement map and R*E + (1-R)*E^2 with a caller-given reflectance). */
enum { UPR_MODEL_IENET_ONLY = 1, UPR_MODEL_HEAD_ONLY = 2 };

typedef struct UprModel UprModel;

/* One state_dict entry: reference key name (e.g. "ie_net.enc1.conv1.weight"),
 * host fp32 data, shape. */
typedef struct {
  const char* name;
  const float* data;
  int ndim;
  int64_t shape[4];
} UprTensorDesc;

/* Replaces constructing + .to(device) + .eval() of MultiScaleUP_Retinex
 * (models/model.py:375-403) / ResidualIENet (:289-331, flag
 * UPR_MODEL_IENET_ONLY): packs an eval-mode state_dict (BatchNorm folded,
 * linear 1x1 chains composed, weights laid out [N][K] in `dtype`) into device
 * memory owned by the handle.  Keys follow the reference state_dict
 * (ResidualIENet keys carry the "ie_net." prefix).  `flags`: 0 or ONE of
 * UPR_MODEL_IENET_ONLY / UPR_MODEL_HEAD_ONLY; unknown bits or both flags
 * return UPR_ERR_ARG before any device call. */
int upr_model_create(const UprTensorDesc* params, int n_params, int use_preact, int use_aspp, int dtype,
                     int flags, UprModel** out);

/* Device bytes of workspace upr_model_forward needs for a B x 3 x H x W batch. */
size_t upr_model_workspace(const UprModel* model, int B, int H, int W);

/* Replaces MultiScaleUP_Retinex.forward (models/model.py:445-455):
 * x [B,3,H,W] in [0,1], H and W multiples of 8 (>= 16)  ->
 * enh [B,3,H,W], refl [B,3,H,W], illu [B,1,H,W] (all `dtype` of the model).
 * With UPR_MODEL_IENET_ONLY (ResidualIENet.forward, :333-360) only `illu` is
 * written and enh/refl may be NULL.  With UPR_MODEL_HEAD_ONLY
 * (multi_scale_enhance(x, reflectance, illu), :415-443) `refl` is an INPUT
 * [B,3,H,W], only `enh` is written and `illu` may be NULL (the reference
 * method does not read it).
 * An fp16 full model forks its multi-scale ops onto an internal side stream
 * after the first conv and joins it before the Retinex tail: completion of
 * `stream` implies completion of the whole forward (env UPR_MS_STREAMS=0: one
 * stream for every model, =1: fp32 models fork too). */
int upr_model_forward(UprModel* model, const void* x, int B, int H, int W, void* enh, void* refl, void* illu,
                      void* workspace, size_t workspace_bytes, void* stream);

void upr_model_destroy(UprModel* model);

/* Number of forwards of this handle so far that ran the two-stream schedule
 * above (0 when every forward stayed on one stream; -1 for NULL).  No
 * reference counterpart: lets a caller report which executor actually ran. */
long long upr_model_forks(const UprModel* model);

/* An fp32 model without PreAct / ASPP runs its convs on the fp16 MFMA unit
 * with fp32 accumulation (about fp32 accuracy), in two ways.  "Split tensors":
 * the convs of the 128- and 256-channel levels (enc2 .. dec3) read and write
 * split-fp16 tensors.  "Split in registers": the 32-channel stride-1 3x3 convs
 * of the row-ring kernel (dec1, the residual head, the EnhancedFAM branch3/4
 * first convs and fusion parts) keep fp32 tensors and split each 8-channel
 * fragment into (hi, lo) fp16 after reading it.  "Weights split once": the
 * 64-wide convs at half resolution (enc1.conv1 / .conv2, dec2.conv.0 / .3)
 * do the same to their activations and read weights the handle split when it
 * was built (upr_pack_split_w_f32).  Env UPR_FP32_SPLIT=0, read by
 * upr_model_create, keeps the fp32 MFMA kernels everywhere; UPR_FP32_SPLIT_REGS=0
 * keeps them for the split-in-registers and weights-split-once ops,
 * UPR_FP32_SPLIT_W64=0 for the weights-split-once ops only.  Of those, the
 * three 64 -> 64 stride-1 convs (enc1.conv2, dec2.conv.0 / .3) run on a row-ring
 * kernel that stages every input row once and splits it once, in LDS; the
 * stride-2 enc1.conv1 runs on a gathered tile that re-stages its rows per tap.
 * UPR_W64_RING=0 (read by upr_model_create; by upr_conv2d_nhwc_wsplit at every
 * call) keeps all four on the gathered tile: the same form code (3), results
 * that differ in rounding only.  The
 * split-in-registers ops convert each element of their LDS row ring to (hi, lo)
 * once, in place: one step before its first reader, beside the MFMAs, or at
 * the top of the step that first reads it, behind a second barrier -- each
 * kernel program in the form that measured faster.  UPR_RING_SPLIT_LDS=0 (read
 * by upr_model_create; by upr_conv2d_nhwc_regs and upr_conv2d_nhwc with
 * UPR_F32_SPLIT_REGS at every call) splits once per filter tap after the LDS
 * read instead; 2 / 3 put every program on the top-of-step / one-step-ahead
 * form (for measurements).  It is the same function on the same values in the
 * same MFMA order, so every setting gives the same bits and the same form
 * code (2); they differ in speed only.  The activations these
 * convs read must stay within the fp16 range (65504): a forward that leaves it
 * sets a flag, and from the next forward on the handle runs the fp32 kernels
 * for good (one line on stderr).  A UPR_MODEL_HEAD_ONLY handle of such a model
 * has no split-tensor op but runs its EnhancedFAM convs split in registers in
 * state 1, as the full model does.  Returns 0: off, 1: active, 2: disabled
 * after an overflow.  No reference counterpart. */
int upr_model_split_state(const UprModel* model);

/* The form every op of the handle's most recent forward ran in, in launch
 * order: 0 = the model dtype's own (exact) kernels, 1 = split tensors, 2 =
 * split in registers, 3 = weights split once.  Fills names[i] (64 bytes each, nullable) and forms[i]
 * for i < max_ops and returns the number of ops (0 before the first forward,
 * -1 for NULL).  No reference counterpart. */
typedef struct {
  char name[64];
  int form;
} UprOpForm;
int upr_model_op_forms(const UprModel* model, UprOpForm* out, int max_ops);

/* Per-op profiling of upr_model_forward (no reference counterpart: the
 * reference only brackets whole calls with time.time(), simple_enhance.py:165-179).
 * enable != 0 records a hipEvent pair around every op of every later forward
 * (stream-ordered, no synchronisation); enable == 0 stops and clears.
 * upr_model_profile_read waits for the recorded events and returns, per op in
 * launch order, the calls, summed device milliseconds, summed GEMM flops
 * (2*M*N*K of the launch) and summed algorithmic bytes. */
enum { UPR_OP_CONV_IGEMM = 0, UPR_OP_OTHER = 1 };
typedef struct {
  char name[64];
  int kind;
  int calls;
  double ms;
  double flops;
  double bytes;
} UprOpStat;
int upr_model_profile(UprModel* model, int enable);
int upr_model_profile_read(UprModel* model, UprOpStat* out, int max_ops, int* n_ops);

const char* upr_status_string(int status);

/* MultiScaleUP_Retinex.retinex_decompose (models/model.py:405-413) on its own:
 * refl = x / (illu + 1e-6) for x [B,C,H,W] and illu [B,illu_c,H,W], illu_c 1
 * (broadcast over C) or C; fp32 arithmetic rounded once to `dtype`.  The
 * backward (autograd of the reference expression) writes dx = g / (illu + 1e-6)
 * and dillu = -sum_c g * x / (illu + 1e-6)^2 (over c when broadcast) into the
 * non-NULL of gx [B,C,H,W] / gillu [B,illu_c,H,W] (overwritten). */
int upr_retinex_decompose(const void* x, const void* illu, void* refl, int B, int C, int H, int W, int illu_c,
                          int dtype, void* stream);
int upr_retinex_decompose_bwd(const void* x, const void* illu, const void* g, void* gx, void* gillu, int B, int C,
                              int H, int W, int illu_c, int dtype, void* stream);

/* Generic NHWC convolution (op-level hook used by the parity tests and by
 * callers composing their own graphs): y = act(conv(x, w) + bias [+ residual]).
 * x [B,H,W,Cin] (Cin % 32 == 0), w packed [Cout][kh*kw*Cin] (tap-major, then
 * channel), bias fp32 [Cout] or NULL, residual [B,Ho,Wo,Cout] or NULL (added
 * before the ReLU), y [B,Ho,Wo,Cout] with Cout % 32 == 0. */
int upr_conv2d_nhwc(const void* x, int B, int H, int W, int Cin, const void* w, const float* bias, int Cout, int kh,
                    int kw, int stride, int pad, int dil, const void* residual, int relu, void* y, int dtype,
                    void* stream);

/* upr_conv2d_nhwc with dtype UPR_F32_SPLIT_REGS runs this with overflow NULL.
 * Arguments as for UPR_F32 (fp32 NHWC x / residual / y, the same packed fp32
 * weights; the weight scales are derived from w).  Only the shapes the
 * split-in-registers kernels take: 3x3, stride 1, pad 1, Cin 32, Cout 32
 * (residual allowed) or 64 (no residual), Ho >= 4, Wo >= 16; anything else
 * returns UPR_ERR_UNSUPPORTED (never another kernel).  `overflow` (device
 * word, nullable) is set to 1 when an input left the fp16 range (|v| >= 65520
 * or non-finite: the outputs are then void); never cleared. */
int upr_conv2d_nhwc_regs(const void* x, int B, int H, int W, int Cin, const void* w, const float* bias, int Cout,
                         int kh, int kw, int stride, int pad, int dil, const void* residual, int relu, void* y,
                         unsigned* overflow, void* stream);

/* Split-fp16 tensors: C fp32 channels of an NHWC pixel stored as 2C fp16,
 * [hi(C) | lo(C)], hi = (half)v, lo = (half)((v - hi) * 2^11); v = hi + lo *
 * 2^-11 to about 2^-22 relative.  upr_split_f32: x fp32 [npix][C] -> y fp16
 * [npix][2C] (C % 8 == 0, 16-byte aligned); `overflow` (device word, nullable)
 * is set to 1 when a |v| > 65504 or non-finite value is met (never cleared).
 * upr_unsplit_f32 is the inverse.  upr_pack_split_f32 (host only): conv weight
 * w fp32 [Cout][Cin][kh][kw] (Cin % 64 == 0) -> the blob upr_conv2d_nhwc takes
 * as `w` with dtype UPR_F32_SPLIT (x, residual and y split tensors, Cout % 128
 * == 0); returns the blob's bytes (0: bad arguments) and fills `out` when
 * out_bytes suffices.  No reference counterpart. */
int upr_split_f32(const float* x, void* y, size_t npix, int C, unsigned* overflow, void* stream);
int upr_unsplit_f32(const void* x, float* y, size_t npix, int C, void* stream);
size_t upr_pack_split_f32(const float* w, int Cout, int Cin, int kh, int kw, void* out, size_t out_bytes);

/* fp32 convs of 64-wide output tiles on the fp16 MFMA unit with the weights
 * split once on the host (tensors stay fp32; every activation fragment is
 * split in registers as in upr_conv2d_nhwc_regs).
 * upr_pack_split_w_f32 (host only): w fp32 in the packed [Cout][kh*kw*Cin]
 * layout upr_conv2d_nhwc takes, optionally followed by a second 1x1 K-segment
 * w2 fp32 [Cout][C2] (NULL / 0: none); Cout % 64 == 0, Cin % 32 == 0, C2 % 32
 * == 0.  Per output channel n, s_n = the power of two that puts the row's
 * max|w| (over both segments) in [2^14, 2^15); the blob holds, per row and per
 * 32 consecutive k, 64 fp16: W_hi = fp16(w s_n) then W_lo = fp16(w s_n -
 * W_hi), each as 4 runs of 8 where run g holds k 4g..4g+3 and 16+4g..16+4g+3
 * (the k-slots of one MFMA lane group); after the planes, at the next multiple
 * of 256 bytes, float 1/s_n [Cout].  Returns the blob's bytes (0: bad
 * arguments) and fills `out` when out_bytes suffices.
 * upr_conv2d_nhwc_wsplit: y = relu?(conv(x) + conv1x1(x2) + bias) + residual
 * (the residual is added after the ReLU), x [B,H,W,Cin], optional second
 * K-segment x2 [B,H2,W2,C2] read at stride2 without padding (NULL: none),
 * residual / y [B,Ho,Wo,Cout], all fp32 NHWC; blob / blob_bytes from
 * upr_pack_split_w_f32 for the same shape (device copy).  Shapes the kernel
 * does not take, or a blob of another size, return UPR_ERR_UNSUPPORTED (never
 * another form).  `overflow` as for upr_conv2d_nhwc_regs.  3x3 stride-1 pad-1
 * ops with Cin = Cout = 64, Ho >= 4, Wo >= 16 (alone, with a residual, or with a
 * 1x1 stride-2 second segment of 32 channels and no residual) run on the
 * row-ring kernel unless UPR_W64_RING=0 is set at the call
 * (UPR_RING_SPLIT_LDS=2 / 3 at the call pick its top-of-step / one-step-ahead
 * schedule); everything else, on the gathered tile.
 * upr_conv_wsplit_ran: which kernel the calling thread's latest
 * upr_conv2d_nhwc_wsplit ran: 0 none (it refused), 1 the gathered tile, 2 the
 * row ring.  No reference counterpart. */
size_t upr_pack_split_w_f32(const float* w, int Cout, int Cin, int kh, int kw, const float* w2, int C2, void* out,
                            size_t out_bytes);
int upr_conv2d_nhwc_wsplit(const void* x, int B, int H, int W, int Cin, const void* blob, size_t blob_bytes,
                           const float* bias, int Cout, int kh, int kw, int stride, int pad, int dil,
                           const void* residual, int relu, void* y, const void* x2, int H2, int W2, int C2,
                           int stride2, unsigned* overflow, void* stream);
int upr_conv_wsplit_ran(void);

/* float -> uint8 exactly as `(x * 255).astype(np.uint8)` on float32
 * (enhancers/adaptive_params.py:142, letterbox.py:93): truncation, wrap mod
 * 256, NaN / |x*255| >= 2^31 -> 0.  n elements, any layout. */
int upr_quantize_u8(const void* x, uint8_t* out, size_t n, int dtype, void* stream);

/* letterbox / letterbox_tensor (utils/letterbox.py:9-102) of ONE image in one
 * launch: src is u8 HWC RGB (src_kind 0) or float32 CHW in [0,1] (src_kind 1,
 * quantised as (x*255).astype(uint8), letterbox.py:93); the H x W source is
 * resized to nh x nw with cv2.resize INTER_LINEAR 8-bit fixed-point semantics
 * (xtab [4][nw], ytab [4][nh] int32: source index 0 / 1, 11-bit weights 0 / 1,
 * built on the host like OpenCV's tables; both NULL when nh == H, nw == W),
 * placed at (top, left) of an Ho x Wo canvas filled with `color`
 * (0xBBGGRR bytes: channel c = (color >> 8c) & 255); out is float32 CHW / 255
 * (out_kind 0, what letterbox_tensor returns) or u8 HWC (out_kind 1). */
int upr_letterbox(const void* src, int src_kind, int H, int W, int top, int left, int nh, int nw, int Ho, int Wo,
                  const int32_t* xtab, const int32_t* ytab, int color, void* out, int out_kind, void* stream);

/* save_image's pixels (enhancers/simple_enhance.py:65-99): one image x [C,H,W]
 * (C = 3, or 1 = replicated to RGB) -> u8 HWC RGB as
 * (np.clip(x, 0, 1) * 255).astype(np.uint8). */
int upr_to_u8_hwc(const void* x, int C, int H, int W, int dtype, uint8_t* out, void* stream);

/* The letterbox of a whole batch in one launch (the batched directory harness,
 * utils/letterbox.py letterbox_u8_batch): image b is described by rec_dev[b]
 * (an array of B records in DEVICE memory) and becomes out[b] of one
 * [B,3,Ho,Wo] tensor.  The arithmetic is upr_letterbox's for src_kind 0 and
 * out_kind 0; dtype UPR_F32 writes those floats (bit-identical), UPR_F16 their
 * fp16 rounding.  Each record must satisfy what upr_letterbox checks of its
 * arguments (top + nh <= Ho, left + nw <= Wo, tables both set or both NULL,
 * NULL only when nh == H and nw == W): the records are not read on the host.
 * src must be 4-byte aligned (the harness aligns every image to 16).
 * UPR_ERR_ARG for B < 1, a NULL pointer or another dtype; nothing is launched. */
typedef struct {
  const uint8_t* src;      /* u8 HWC RGB, H x W, on the device */
  const int32_t* xtab;     /* [4][nw], NULL when nw == W && nh == H */
  const int32_t* ytab;     /* [4][nh] */
  int32_t H, W, top, left, nh, nw;
} upr_letterbox_rec;

int upr_letterbox_batch(const upr_letterbox_rec* rec_dev, int B, int Ho, int Wo, int color,
                        void* out /* [B,3,Ho,Wo] */, int dtype, void* stream);

/* The pixels of the harness's three output files for a whole batch in one
 * pass: x, enh [B,3,H,W] and illu [B,1,H,W] (NULL: none) of one dtype ->
 * enh_u8 [B,H,W,3], illu_u8 [B,H,W,3] (the map replicated to RGB; NULL: not
 * written) and cmp_u8 [B,H,cmp_panels*W,3] (NULL: not written): the panels
 * [x | enh] (cmp_panels 2) or [x | enh | illu] (3) side by side.  Every byte is
 * upr_to_u8_hwc's.  UPR_ERR_ARG for B < 1, NULL x / enh / enh_u8, an output
 * that needs illu without it, cmp_panels other than 2 / 3 with cmp_u8. */
int upr_panels_u8(const void* x, const void* enh, const void* illu /* [B,1,H,W] or NULL */, int B, int H, int W,
                  int dtype, uint8_t* enh_u8 /* [B,H,W,3] */, uint8_t* illu_u8 /* [B,H,W,3] or NULL */,
                  uint8_t* cmp_u8 /* [B,H,P*W,3] or NULL */, int cmp_panels /* 2 or 3 */, void* stream);

/* cv2.cvtColor(..., COLOR_RGB2LAB) / (..., COLOR_LAB2RGB) on 8-bit interleaved
 * pixels (adaptive_params.py:142-145, :158-161 — the reference goes through
 * BGR, which is the same arithmetic). */
int upr_rgb2lab_u8(const uint8_t* rgb, uint8_t* lab, size_t npix, void* stream);
int upr_lab2rgb_u8(const uint8_t* lab, uint8_t* rgb, size_t npix, void* stream);

/* cv2.createCLAHE(clip, (tiles_x, tiles_y)).apply on B planar 8-bit images
 * [B,H,W] (adaptive_params.py:149-152).  lut_ws: B*tiles_x*tiles_y*256 bytes. */
int upr_clahe_u8(const uint8_t* src, uint8_t* dst, uint8_t* lut_ws, int B, int H, int W, float clip, int tiles_x,
                 int tiles_y, void* stream);

/* Fused AdaptiveParameterAdjuster.apply_clahe_enhancement
 * (adaptive_params.py:121-169) on a batch: enh [B,3,H,W] float -> quantise ->
 * Lab -> CLAHE(clip, tiles) on L -> RGB -> /255 -> out [B,3,H,W].
 * Workspace: upr_clahe_enhance_workspace() bytes. */
size_t upr_clahe_enhance_workspace(int B, int H, int W, int tiles_x, int tiles_y);
int upr_clahe_enhance(const void* enh, void* out, void* workspace, int B, int H, int W, float clip, int tiles_x,
                      int tiles_y, int dtype, void* stream);

/* 256-bin histogram of the 8-bit BGR2GRAY image of each x [B,3,H,W] float
 * (calculate_brightness_features, adaptive_params.py:24-68): hist int32 [B,256]. */
int upr_gray_hist(const void* x, int32_t* hist, int B, int H, int W, int dtype, void* stream);

/* MultiScaleEnhancer (enhancers/multi_scale.py:17-115) per image:
 * sums fp64 [B,3] = per-scale feature sums; factor fp64 [B] (nullable);
 * when enh/out are non-NULL, out = clamp(enh * factor, 0, 1). */
int upr_multiscale(const void* x, const void* enh, void* out, double* sums, double* factor, int B, int H, int W,
                   int dtype, void* stream);

/* MultiScaleEnhancer.extract_multi_scale_features (multi_scale.py:17-60), one
 * scale (0: x1, 1: x0.5, 2: x0.25, size int(h*s) x int(w*s)):
 * out [B,7,hs,ws] = [bilinear image (3), luminance, gradient magnitude (3)]. */
int upr_multiscale_features(const void* x, void* out, int B, int H, int W, int scale_idx, int dtype, void* stream);

/* ContentAwareEnhancer (enhancers/content_aware.py:19-122) per image of
 * x [B,3,H,W]: saliency fp32 [B,H,W] (compute_saliency_map, nullable),
 * attention fp32 [B,H,W] (compute_attention_map, nullable) and, when enh/out
 * are non-NULL, out = clamp(enh * (1 + 0.2 * attention), 0, 1)
 * (apply_content_aware_enhancement :93-122, all on the device — the
 * reference's saliency stays on the CPU, :56-57). */
size_t upr_content_aware_workspace(int B, int H, int W);
int upr_content_aware(const void* x, const void* enh, void* out, float* saliency, float* attention, void* workspace,
                      size_t workspace_bytes, int B, int H, int W, int dtype, void* stream);

/* calculate_metrics with calculate_psnr / calculate_ssim / calculate_niqe /
 * calculate_saturation / calculate_naturalness (utils/utils.py:95-333) for every
 * image of enh [B,3,H,W] (H, W >= 8); `ref` (the ground truth, same shape and
 * dtype) may be NULL.  The reference takes one image per call on the host;
 * here each image of the batch is measured on its own, and its result does
 * not depend on B or on its position.  fp16 input is widened to fp32 exactly.
 * metrics fp64 [B][UPR_METRICS_N], in the order of the UPR_METRIC_* indices:
 * mean_brightness, contrast (:125-130), entropy (np.histogram, 256 bins over
 * [0,1], :133-137), niqe (:250-278; gray and gray^2 in float32, the 7x7 means
 * in fp64 with scipy's `reflect` border, sigma = sqrt(max(E[g^2] - mu^2, 0)) --
 * the reference yields NaN where float32 rounding makes a flat window's
 * variance negative), saturation (:281-303), naturalness (:306-333), then mse
 * (:170), psnr (:186-202) and ssim (:205-247; 11x11 box means in fp64, zero
 * border, divisor 121), the last three NaN when ref is NULL.
 * sums fp64 [B][UPR_METRICS_NSUMS] (nullable), the raw per-image sums:
 * 0-2 sum x per channel, 3-5 sum x^2 per channel, 6 sum of the per-pixel
 * saturation, 7 sum sigma, 8 sum mu, 9 sum mu^2 (NIQE), 10 sum (x - y)^2 over
 * the three channels, 11-13 sum of the SSIM map per channel (10-13 NaN when
 * ref is NULL).  hist int32 [B,256] (nullable): the entropy's histogram.
 * Sums are added in a fixed order: a rerun gives the same bits. */
enum { UPR_METRICS_N = 9, UPR_METRICS_NSUMS = 14 };
enum {
  UPR_METRIC_MEAN_BRIGHTNESS = 0,
  UPR_METRIC_CONTRAST = 1,
  UPR_METRIC_ENTROPY = 2,
  UPR_METRIC_NIQE = 3,
  UPR_METRIC_SATURATION = 4,
  UPR_METRIC_NATURALNESS = 5,
  UPR_METRIC_MSE = 6,
  UPR_METRIC_PSNR = 7,
  UPR_METRIC_SSIM = 8
};
size_t upr_image_metrics_workspace(int B, int H, int W);
int upr_image_metrics(const void* enh, const void* ref, double* metrics, double* sums, int32_t* hist,
                      void* workspace, size_t workspace_bytes, int B, int H, int W, int dtype, void* stream);

/* Lightness order error (LOE; S. Wang, J. Zheng, H.-M. Hu, B. Li, "Naturalness
 * preserved enhancement algorithm for non-uniform illumination images", IEEE
 * Trans. Image Processing 22(9), 2013) of enh against its own low-light input
 * low, both [B,3,H,W] of one dtype (H, W >= 1, H * W < 2^31), per image; no
 * ground truth is involved and the reference has no counterpart.  Integer and
 * exact:
 *   q(v)   upr_to_u8_hwc's cast: clamp to [0, 1], times 255 in float32,
 *          truncated (fp16 input widened exactly first)
 *   L(p)   max(q(R), q(G), q(B)), 0..255
 *   grid   with m = min(H, W): every pixel when sample == 0 or m <= sample,
 *          else h x w pixels, h = max(1, (H * sample + m / 2) / m) and w
 *          likewise (integer division); grid row i is source row
 *          ((2 i + 1) * H) / (2 h), columns likewise; N = h * w
 *   D      the ordered pairs (x, y) of grid pixels with
 *          (L_low(x) >= L_low(y)) != (L_enh(x) >= L_enh(y))
 *   loe    D / N as one fp64 division (the paper's mean relative-order
 *          difference); sample = 50 is the literature's convention
 * D is taken from the 256 x 256 joint histogram of (L_low, L_enh) and its 2-D
 * prefix, never pair by pair.  loe fp64 [B]; counts int64 [B][2] = (D, N),
 * nullable.  Image b's result does not depend on B or its position, and every
 * sum is an integer sum: a rerun gives the same bits.  The workspace
 * (upr_image_loe_workspace(B) bytes: two int32 tables per image) is zeroed by
 * the call itself on `stream`; a caller may reuse one across calls. */
size_t upr_image_loe_workspace(int B);
int upr_image_loe(const void* low, const void* enh, double* loe, int64_t* counts, void* workspace,
                  size_t workspace_bytes, int B, int H, int W, int sample, int dtype, void* stream);

/* Lossless 8-bit RGB PNG files written entirely on the device (no reference
 * counterpart: the reference saves through PIL on the host).  hwc_u8 is B
 * images u8 [H,W,3]; image b's complete file is written contiguously at out +
 * b * out_stride and its length to sizes[b] (device int64), so the host only
 * copies sizes[b] bytes and writes them.  The file: signature, IHDR (bit depth
 * 8, colour type 2, no interlace), one IDAT per strip of rows_per_strip rows
 * (clamped to H; the last strip may be shorter), a trailing IDAT with the
 * Adler-32, IEND.  A strip is one deflate block of dynamic Huffman codes over
 * literals and end-of-block only (code lengths <= 15 bits, no LZ77 matches,
 * no run symbols in the code-length alphabet, HDIST 0 with a distance code of
 * length 0) followed by an empty stored block, or, when that would be no
 * smaller, stored blocks of at most 65535 bytes: a file never exceeds
 * bytes_per_image.  `filter` is a UPR_PNG_FILTER_* value; ADAPTIVE takes per
 * row the type with the smallest sum of min(v, 256 - v) over the filtered
 * bytes (ties: the lowest type).  Filters see raw pixels: the row above a
 * strip's first row is the image row above it.  All checksums (CRC-32 of every
 * chunk, Adler-32) are computed on the device; the output is a function of
 * the pixels and the arguments only.
 * upr_png_bound: the largest file of one H x W image (out_stride must be at
 * least that) and the scratch bytes per image (upr_png_encode needs B times
 * that, 16-byte aligned).  UPR_ERR_SHAPE, with nothing launched, when
 * rows_per_strip * (3 W + 1) > UPR_PNG_MAX_STRIP_BYTES or bytes_per_image
 * would exceed 2^31.
 * The _ex forms take a match mode; upr_png_bound and upr_png_encode are the
 * _ex forms with UPR_PNG_MATCH_NONE, the file described above.  With
 * UPR_PNG_MATCH_LZ a strip's filtered bytes are also parsed greedily into
 * literals and LZ77 matches (length 3..258, distance 1..32768, never reaching
 * before the strip's first filtered byte, so each IDAT payload stays an
 * independent deflate stream on a byte boundary), coded with a literal/length
 * and a distance code (<= 15 bits, HLIT and HDIST as used, extra bits as in
 * RFC 1951 3.2.5), and the strip is written in the smallest of three forms:
 * that block, the literal-only block, stored blocks.  No strip is larger than
 * with MATCH_NONE, so bytes_per_image is the same; scratch_bytes grows by the
 * staged filtered bytes and one 32-bit match word per filtered byte.  The
 * output is still a function of the pixels and the arguments only.  A match
 * value other than the two is UPR_ERR_ARG. */
enum {
  UPR_PNG_FILTER_NONE = 0,
  UPR_PNG_FILTER_SUB = 1,
  UPR_PNG_FILTER_UP = 2,
  UPR_PNG_FILTER_AVG = 3,
  UPR_PNG_FILTER_PAETH = 4,
  UPR_PNG_FILTER_ADAPTIVE = 5
};
enum { UPR_PNG_MAX_STRIP_BYTES = 1 << 24 };
enum { UPR_PNG_MATCH_NONE = 0, UPR_PNG_MATCH_LZ = 1 };
int upr_png_bound(int H, int W, int rows_per_strip, size_t* bytes_per_image, size_t* scratch_bytes);
int upr_png_bound_ex(int H, int W, int rows_per_strip, int match, size_t* bytes_per_image, size_t* scratch_bytes);
int upr_png_encode_ex(const uint8_t* hwc_u8, int B, int H, int W, int filter, int match, int rows_per_strip,
                      uint8_t* out, size_t out_stride, int64_t* sizes, void* scratch, size_t scratch_bytes,
                      void* stream);
int upr_png_encode(const uint8_t* hwc_u8, int B, int H, int W, int filter, int rows_per_strip, uint8_t* out,
                   size_t out_stride, int64_t* sizes, void* scratch, size_t scratch_bytes, void* stream);

/* Baseline JPEG files written entirely on the device (no reference
 * counterpart).  Arguments as upr_png_encode: hwc_u8 is B images u8 [H,W,3];
 * image b's complete file is written at out + b * out_stride and its length to
 * sizes[b] (device int64).  The file: SOI, APP0 JFIF 1.01, DQT 0 (luma) and 1
 * (chroma), SOF0 (8-bit, Y/Cb/Cr, every component 1x1: 4:4:4), the four
 * Annex K Huffman tables (DHT DC0, AC0, DC1, AC1), DRI, SOS, the entropy-coded
 * data, EOI.  `quality` is 1..100 and scales the Annex K quantisation tables
 * the libjpeg way (scale = 5000 / Q below 50, else 200 - 2 Q; q = clamp((base
 * scale + 50) / 100, 1, 255)).  A restart interval is restart_rows rows of 8x8
 * blocks (clamped to the image; DRI's Ri = ceil(W / 8) restart_rows), RSTm (m
 * = interval mod 8) behind every interval but the last.  H and W are padded to
 * multiples of 8 by repeating the last row / column.  Colour conversion, the
 * forward DCT and the quantisation are integer arithmetic, stated in
 * the output is a function of the pixels and the arguments
 * only.  upr_jpeg_encode / upr_jpeg_bound are the _ex forms below with
 * (UPR_JPEG_444, UPR_JPEG_HUFF_STANDARD).  Not built: 4:2:2, progressive
 * scans, arithmetic coding.
 * upr_jpeg_bound: the largest file of one H x W image (out_stride must be at
 * least that) and the scratch bytes per image (upr_jpeg_encode needs B times
 * that, 16-byte aligned).  The bound comes from the code tables: a block is at
 * most (longest DC code, 11) + 11 + 63 ((longest AC code, 16) + 10) = 22 + 63
 * * 26 = 1660 bits; an interval of n blocks (n = 3 ceil(W / 8) times its block
 * rows) at most 2 ceil(1660 n / 8) + 2 bytes (doubled for the 0x00 behind
 * every 0xFF, 2 for the marker behind it); the file UPR_JPEG_HEADER_BYTES plus
 * its intervals: about 6.5 times the raw pixels.
 * UPR_ERR_SHAPE, with nothing launched, when H or W > 65535, Ri > 65535 or
 * bytes_per_image would exceed 2^31; UPR_ERR_ARG for a null pointer, B, H, W
 * or restart_rows <= 0, a quality outside 1..100, an out_stride below
 * bytes_per_image or a misaligned scratch; UPR_ERR_WORKSPACE for too little
 * scratch. */
enum { UPR_JPEG_HEADER_BYTES = 629, UPR_JPEG_MAX_BLOCK_BITS = 1660 };
int upr_jpeg_bound(int H, int W, int restart_rows, size_t* bytes_per_image, size_t* scratch_bytes);
int upr_jpeg_encode(const uint8_t* hwc_u8, int B, int H, int W, int quality, int restart_rows, uint8_t* out,
                    size_t out_stride, int64_t* sizes, void* scratch, size_t scratch_bytes, void* stream);

/* The encoder's further modes.  Everything above holds (colour formulae, DCT,
 * quantisation, entropy coding rules, stuffing, 1-padding, RSTm, DRI always
 * written); restart_rows counts MCU rows in every mode and Ri = MCUs per row
 * x restart_rows, clamped to the image, at most 65535.
 * subsampling:
 *   UPR_JPEG_444   the file of upr_jpeg_encode; an MCU is 8x8 pixels, Y Cb Cr.
 *   UPR_JPEG_420   H and W are padded to multiples of 16 by repeating the last
 *                  row / column; Y, Cb, Cr (0..255) per pixel by the formulae
 *                  above; a chroma sample is the 2x2 box (a + b + c + d + 2)
 *                  >> 2, then minus 128.  SOF0 sampling factors Y 0x22, Cb
 *                  0x11, Cr 0x11; an MCU is 16x16 pixels, blocks Y00 Y01 Y10
 *                  Y11 Cb Cr, one DC predictor per component.
 *   UPR_JPEG_GRAY  one component: Y of the [H,W,3] input by the formula above
 *                  (exactly v for R = G = B = v).  SOF0 Nf 1 (id 1, 0x11, Tq
 *                  0), DQT 0 alone, DHT DC0 and AC0 alone, SOS Ns 1; an MCU is
 *                  one 8x8 block, blocks in raster order.
 * huffman:
 *   UPR_JPEG_HUFF_STANDARD   the Annex K tables.
 *   UPR_JPEG_HUFF_OPTIMIZED  tables of each image's own: DC0 / AC0 for Y, DC1
 *     / AC1 for Cb + Cr.  Per table: the exact count of every symbol the
 *     image's coding emits over all its intervals (DC categories; AC (run,
 *     size), ZRL, EOB); while the counts' total exceeds 2^22 every non-zero
 *     count f becomes (f + 1) >> 1 (merge depth <= 31); Annex K.2 as libjpeg's
 *     jpeg_gen_optimal_table states it on 257 entries with freq[256] = 1 (c1
 *     the smallest non-zero count, ties to the largest index; c2 the next
 *     smallest other than c1, ties to the largest index; c2 merges into c1,
 *     codesize incremented along both `others` chains; until there is no c2);
 *     bits[codesize[i]]++; the Figure K.3 limit for i = 32 .. 17 (while
 *     bits[i] > 0: j from i - 2 down to the first with bits[j] > 0; bits[i]
 *     -= 2, bits[i-1]++, bits[j+1] += 2, bits[j]--); the longest non-empty
 *     length is decremented once (the reserved entry: no code is all ones);
 *     HUFFVAL in the order len = 1..32, sym = 0..255 with codesize[sym] ==
 *     len; canonical codes (Annex C).  A table with one used symbol has one
 *     1-bit code.  A DHT segment is 19 + nvals bytes behind its marker, so
 *     the header's length varies per image.
 * upr_jpeg_bound_ex: as upr_jpeg_bound with a block at most
 * UPR_JPEG_MAX_BLOCK_BITS (standard) or (16 + 11) + 63 (16 + 10) =
 * UPR_JPEG_MAX_BLOCK_BITS_OPTIMIZED bits, n = units per MCU (3, 6, 1) x MCUs
 * per row x the interval's MCU rows, and the header UPR_JPEG_HEADER_BYTES
 * (UPR_JPEG_HEADER_BYTES_GRAY for gray; an optimised DHT is never longer than
 * the Annex K one: at most 12 DC and 162 AC symbols exist).  The scratch of
 * the optimised mode also holds the image's counts and tables.
 * Errors as above; an unknown subsampling or huffman value is UPR_ERR_ARG.
 * upr_jpeg_huffman_build: the encoder's table routine on caller-supplied
 * counts: freq is n tables of 257 u32 (entry 256 is ignored: the reserved
 * entry is always 1) on the device; table t's BITS[16] then HUFFVAL[256]
 * (zero behind nvals[t]) go to bits_vals + 272 t, the number of coded symbols
 * to nvals[t]; all-zero counts give nvals 0.  UPR_ERR_ARG for a null pointer
 * or n <= 0. */
enum { UPR_JPEG_444 = 0, UPR_JPEG_420 = 1, UPR_JPEG_GRAY = 2 };
enum { UPR_JPEG_HUFF_STANDARD = 0, UPR_JPEG_HUFF_OPTIMIZED = 1 };
enum { UPR_JPEG_HEADER_BYTES_GRAY = 334, UPR_JPEG_MAX_BLOCK_BITS_OPTIMIZED = 1665 };
int upr_jpeg_bound_ex(int H, int W, int restart_rows, int subsampling, int huffman, size_t* bytes_per_image,
                      size_t* scratch_bytes);
int upr_jpeg_encode_ex(const uint8_t* hwc_u8, int B, int H, int W, int quality, int restart_rows, int subsampling,
                       int huffman, uint8_t* out, size_t out_stride, int64_t* sizes, void* scratch,
                       size_t scratch_bytes, void* stream);
int upr_jpeg_huffman_build(const uint32_t* freq, int n, uint8_t* bits_vals, int32_t* nvals, void* stream);

/* Guided-filter restore of the letterboxed result to the source's size (the
 * fast guided filter of He & Sun 2015, per channel; no reference counterpart:
 * the reference records original_size and never uses it).  All pixel values
 * are in 0..255 units; the arithmetic is stated exactly, and the device agrees
 * with a numpy restatement byte for byte (tests/guided_ref.py).
 *
 * upr_guided_fit: guide_u8 and target_u8 are u8 [B,Hl,Wl,3], the letterboxed
 * input and result as the output files hold them; only the content rectangle
 * (top, left, nh, nw) of either is read.  Per image, channel c and content
 * pixel (y, x), with the window of `radius` clipped to the content rectangle:
 *   N (count), S_I, S_p, S_II, S_Ip: exact integer sums over the window of
 *     I = guide[..., c] and p = target[..., c] (int32; the products in int64)
 *   num = (double)(N S_Ip - S_I S_p)
 *   den = (double)(N S_II - S_I S_I) + (eps * 65025.0) * (double)(N N)
 *   a = num / den,  b = ((double)S_p - a (double)S_I) / (double)N
 * in fp64, one operation at a time, no contraction.  The coefficient maps are
 * the clipped window means A = hsum_then_vsum(a) / (double)N and B likewise:
 * a pixel's row sum adds its in-range taps in increasing x starting from the
 * first one, the column sum adds those row sums in increasing y (no running
 * sums that subtract).  ab: fp64 [B,2,3,nh,nw] (A's three planes, then B's).
 * workspace: upr_guided_fit_workspace(B, nh, nw) bytes (the a, b maps).
 *
 * upr_guided_apply: src_u8 is B u8 HWC images of one H x W, image b at
 * src_u8 + b * src_stride (bytes, >= 3 H W; any alignment, the harness stages
 * at multiples of 16).  Per full-resolution pixel (Y, X):
 *   fy = ((double)Y + 0.5) * ((double)nh / (double)H) - 0.5, clamped to
 *     [0, nh - 1]; y0 = floor(fy), y1 = min(y0 + 1, nh - 1), wy = fy - y0;
 *     the same in x
 *   v(M) = (1 - wy) ((1 - wx) M00 + wx M01) + wy ((1 - wx) M10 + wx M11)
 *   enh = (uint8)floor(min(max(v(A) src + v(B), 0), 255) + 0.5)
 * illu_lb_u8 (NULL: none) is the letterboxed illumination file's pixels, u8
 * [B,Hl,Wl,3]; the map is not fitted: its full-resolution pixels are the same
 * bilinear sample of channel 0 of its content pixels, floor(v(illu) + 0.5),
 * replicated to RGB.  Outputs: enh_u8 [B,H,W,3], illu_u8 [B,H,W,3] (NULL: not
 * written) and cmp_u8 [B,H,cmp_panels*W,3] (NULL: not written), the panels
 * [src | enh] (2) or [src | enh | illu] (3) as in upr_panels_u8.  One pass:
 * every source byte is read once, every output byte written once.
 *
 * Both: UPR_ERR_ARG, with nothing launched, for a NULL guide / target / ab /
 * workspace / src / enh_u8, B < 1, a content rectangle outside Hl x Wl, radius
 * outside 1..32, eps <= 0, an output that needs illu_lb_u8 without it,
 * cmp_panels other than 2 / 3 with cmp_u8, src_stride < 3 H W; UPR_ERR_SHAPE
 * for nh > H or nw > W (the restore never shrinks) or B beyond one launch's
 * grid (10922 fit, 65535 apply); UPR_ERR_WORKSPACE for too little workspace. */
size_t upr_guided_fit_workspace(int B, int nh, int nw);
int upr_guided_fit(const uint8_t* guide_u8, const uint8_t* target_u8, int B, int Hl, int Wl, int top, int left,
                   int nh, int nw, int radius, double eps, double* ab /* [B,2,3,nh,nw] */, void* workspace,
                   size_t workspace_bytes, void* stream);
int upr_guided_apply(const uint8_t* src_u8, size_t src_stride, int B, int H, int W, const double* ab,
                     const uint8_t* illu_lb_u8 /* [B,Hl,Wl,3] or NULL */, int Hl, int Wl, int top, int left, int nh,
                     int nw, uint8_t* enh_u8 /* [B,H,W,3] */, uint8_t* illu_u8 /* [B,H,W,3] or NULL */,
                     uint8_t* cmp_u8 /* [B,H,P*W,3] or NULL */, int cmp_panels /* 2 or 3 */, void* stream);

/* Non-local means on the u8 pixels of an output file, the filter strength per
 * pixel from the u8 illumination map (the Retinex gain ~ 1 / illumination
 * amplifies the sensor noise by the same factor; no reference counterpart).
 * Integers throughout: the device agrees with a numpy restatement byte for
 * byte (tests/denoise_ref.py).
 *
 * upr_denoise_lut (host only, no device call): the strength table of a
 * (strength, floor, patch) triple, fp64 one operation at a time, with
 * n = 3 (2 patch + 1)^2 and L = 0..255:
 *   h = strength * 255.0 / (double)max(L, floor);  h2 = h * h
 *   lut[L] = (uint32)min(floor(1048576.0 * 32.0 / ((double)n * h2) + 0.5), 4294967295.0)
 *   lut[L] = 4294967295 when h2 == 0
 * strength is the assumed noise std of the input in u8 levels before the
 * enhancement gain.  UPR_ERR_ARG for a NULL lut, strength < 0 or not a number,
 * floor outside 1..255, patch outside 1..3.
 *
 * upr_denoise_nlm_u8: src_u8 and out_u8 are u8 [B,H,W,3]; illu_u8 (NULL: L =
 * 255 everywhere) is the illumination file's pixels, u8 with a pixel stride of
 * illu_stride = 1 ([B,H,W]) or 3 ([B,H,W,3], channel 0 is read) bytes.  Only
 * the content rectangle (top, left, nh, nw) is filtered; the pixels outside it
 * are copied.  I~(y, x) is src at coordinates clamped to the rectangle.  For a
 * content pixel p and every candidate q = p + s, |s_y|, |s_x| <= search, that
 * lies inside the rectangle (the others are skipped):
 *   d = sum over |o_y|, |o_x| <= patch and c of (I~_c(p + o) - I~_c(q + o))^2
 *     (an exact integer, <= 147 * 255^2 < 2^24)
 *   t = ((uint64)d * lut[L(p)]) >> 20          (t / 32 = mean sq. difference / h^2)
 *   w = EXPW[t] for t < 256, else 0;  EXPW[i] = floor(4095 exp(-i / 32) + 0.5),
 *     256 literal integers 4095, 3969, 3847, 3729 ... 2, 2, 1, 1
 *   out_c(p) = (2 sum(w I_c(q)) + sum(w)) / (2 sum(w))   (integer division)
 * The centre candidate contributes 4095, so sum(w) > 0; every sum fits int32.
 * No workspace.  UPR_ERR_ARG, with nothing launched, for a NULL src / out /
 * lut, out_u8 == src_u8 or overlapping it, B < 1, a content rectangle outside
 * H x W, search outside 1..10, patch outside 1..3, illu_stride other than 1 /
 * 3 with a map; UPR_ERR_SHAPE for B > 65535. */
int upr_denoise_lut(double strength, int floor, int patch, uint32_t* lut /* [256] */);
int upr_denoise_nlm_u8(const uint8_t* src_u8, const uint8_t* illu_u8 /* or NULL */, int illu_stride, int B, int H,
                       int W, int top, int left, int nh, int nw, int search, int patch,
                       const uint32_t* lut /* [256], host */, uint8_t* out_u8, void* stream);

/* Blind denoising: the noise level of each image measured on the device, a
 * strength table per image built from it, and the filter reading those tables
 * (no host round trip; tests/noise_ref.py restates all three, bit for bit).
 *
 * upr_noise_sigma_u8: the Laplacian-difference estimator (Immerkaer 1996) with
 * a median.  src_u8 is u8 [B,H,W,3], the letterboxed low-light INPUT's pixels
 * (not the enhanced image's), with the content rectangle (top, left, nh, nw).
 * For every channel c and interior content pixel 1 <= y <= nh-2, 1 <= x <= nw-2
 * (content coordinates; nothing is clamped, no pixel outside the rectangle
 * counts):
 *   r = I(y-1,x-1) + I(y-1,x+1) + I(y+1,x-1) + I(y+1,x+1)
 *       - 2 (I(y-1,x) + I(y+1,x) + I(y,x-1) + I(y,x+1)) + 4 I(y,x)      |r| <= 2040
 *   the sample is skipped when one of its nine values is 0 or 255 (clipped
 *   pixels understate the noise), else hist[|r|] += 1: one histogram of 2041
 *   uint32 counts per image, the three channels pooled.
 * Independent noise of std s gives r a std of 6 s (the squared coefficients
 * sum to 36).  Then, per image:
 *   n = sum(hist);  sigma = 0 when n == 0, else
 *   b = the smallest bin with 2 cum(b) >= n, below = cum(b - 1) (0 for b = 0)
 *   (lo, wd) = (b - 0.5, 1.0), or (0.0, 0.5) for b = 0
 *   frac = (double)(n - 2 below) / (double)(2 hist[b])
 *   med = lo + wd * frac;  sigma = med / 4.0469385011764905   (6 x 0.6744897501960817)
 * in fp64, one operation at a time.  sigma: double [B] on the device.
 * workspace: upr_noise_sigma_workspace(B) bytes, 16-byte aligned; the call
 * zeroes it itself.  A rectangle with nh < 3 or nw < 3 is legal: sigma = 0.
 * UPR_ERR_ARG, with nothing launched, for a NULL src / sigma / workspace (or a
 * misaligned one), B < 1, a rectangle outside H x W; UPR_ERR_SHAPE for
 * 3 nh nw >= 2^31 or B > 65535; UPR_ERR_WORKSPACE for too little workspace.
 *
 * upr_denoise_lut_dev: lut[b] = upr_denoise_lut(scale * sigma[b], floor, patch)
 * for every image, entry for entry (the same fp64 steps, the h2 == 0 entry
 * included), one launch of B x 256 threads.  UPR_ERR_ARG as upr_denoise_lut,
 * and for a NULL sigma, B < 1, scale < 0 or not finite.
 *
 * upr_denoise_nlm_u8_luts: upr_denoise_nlm_u8 with `luts` a DEVICE pointer to
 * uint32 [B,256]; image b is filtered with row b.  Everything else, errors
 * included, as upr_denoise_nlm_u8. */
size_t upr_noise_sigma_workspace(int B);
int upr_noise_sigma_u8(const uint8_t* src_u8, int B, int H, int W, int top, int left, int nh, int nw,
                       double* sigma /* [B], device */, void* workspace, size_t workspace_bytes, void* stream);
int upr_denoise_lut_dev(const double* sigma /* [B], device */, int B, double scale, int floor, int patch,
                        uint32_t* lut /* [B,256], device */, void* stream);
int upr_denoise_nlm_u8_luts(const uint8_t* src_u8, const uint8_t* illu_u8 /* or NULL */, int illu_stride, int B, int H,
                            int W, int top, int left, int nh, int nw, int search, int patch,
                            const uint32_t* luts /* [B,256], device */, uint8_t* out_u8, void* stream);

/* Host copies of the 8-bit Lab integer tables (for CPU-side verification):
 * gamma[256], cbrt[3072], yf[512], invgamma[4096] (uint16), rgb2xyz[9], xyz2rgb[9]. */
void upr_lab_tables(uint16_t* gamma, uint16_t* cbrt, uint16_t* yf, uint16_t* invgamma, int32_t* rgb2xyz,
                    int32_t* xyz2rgb);

/* Measured ceilings for the bench's roofline report (bench.py --ceilings; not
 * on the model path).  Runs `reps` back-to-back launches of `blocks` 256-thread
 * workgroups on `stream` and returns the average milliseconds per launch:
 *   UPR_CALIB_MFMA_F16: `iters` x 8 v_mfma_f32_16x16x32_f16 per wave on random
 *     fp16 operands held in registers (FLOPs = blocks * 4 * iters * 8 * 16384);
 *     src >= 1 MiB of fp16 (bytes), dst = blocks * 256 * 4 floats;
 *   UPR_CALIB_HBM_COPY: dst[0:bytes] = src[0:bytes], 16 B per lane (HBM bytes =
 *     2 * bytes; 16-byte aligned); iters selects the access form: 0 grid-stride,
 *     1 grid-stride non-temporal, 2 one contiguous slice per workgroup.
 * Stands in for no reference interface: the reference has no roofline. */
enum { UPR_CALIB_MFMA_F16 = 0, UPR_CALIB_HBM_COPY = 1 };
int upr_calib_run(int which, int blocks, int iters, const void* src, void* dst, size_t bytes, int reps,
                  float* ms_per_launch, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* UPR_H_ */
