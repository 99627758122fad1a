// Shared definitions for the UP-Retinex gfx950 kernel library (libupr.so).
//
// Activations live in HBM as NHWC (channels innermost) in the model's storage
// type T (float or _Float16); accumulation is always fp32.  The C ABI itself
// (include/upr.h) exposes only plain pointers, sizes and a stream handle.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>

#define UPR_CHECK_HIP(expr)                                  \
  do {                                                       \
    hipError_t _e = (expr);                                  \
    if (_e != hipSuccess) return (int)_e;                    \
  } while (0)

namespace upr {

typedef _Float16 half_t;

// Status codes (mirrored in include/upr.h).
enum : int {
  kOk = 0,
  kErrArg = -1,
  kErrShape = -2,
  kErrMissingParam = -3,
  kErrWorkspace = -4,
  kErrUnsupported = -5,
};

enum DType : int { kF32 = 0, kF16 = 1 };

// ---------------------------------------------------------------------------
// Implicit-GEMM convolution descriptor.
//
// GEMM view: M = B*Ho*Wo output pixels, N = output channels, K = sum over
// segments of (kh*kw*C_seg).  A segment is one operand of a "virtual concat":
// it reads C channels of an NHWC source at channel offset coff (pixel stride
// cs), through a kh x kw window with its own stride / padding / dilation.  The
// packed weight matrix is [N][Kpad] (k contiguous), K ordered (segment, tap,
// channel).
// ---------------------------------------------------------------------------
enum SegPre : int {
  kPreNone = 0,
  kPreAffineRelu = 1,  // v = max(v*pre_scale[c] + pre_shift[c], 0), in-bounds taps only
  kPreMaxPool3 = 2,    // 3x3/s1/p1 max-pool of the source (padding ignored), then the tap
};

struct ConvSeg {
  const void* src;
  int C, cs, coff;      // channels read, source pixel stride, channel offset
  int Hin, Win;
  int kh, kw, stride, pad, dil;
  int pre;
  const float* pre_scale;
  const float* pre_shift;
  int kbase;            // first k row of this segment in the packed weights
};

enum StoreMode : int {
  kStoreNHWC = 0,       // out[m*out_cs + out_coff + n]
  kStoreConvT2x2 = 1,   // ConvTranspose2d k2 s2 pixel shuffle: n = (dy*2+dx)*Cout + co
  kStoreHeadIllu = 2,   // residual head: illu = sigmoid(mean_c(x) + relu(v).w2 + b2) (N == 32)
};

struct ConvOp {
  int nseg;
  ConvSeg seg[4];
  int B, Ho, Wo, N;
  int Kpad;
  const void* W;          // packed weights [N][Kpad], type T
  const float* scale;     // per output channel (nullable => 1)
  const float* bias;      // per output channel (nullable => 0)
  const float* img_bias;  // per (image, channel) [B][N] (nullable)
  const void* res1; int res1_cs;  // added before ReLU (nullable)
  int relu;
  const void* res2; int res2_cs;  // added after ReLU (nullable)
  void* out; int out_cs, out_coff;
  int store;
  float* pool;            // per (image, channel) sum of the stored value (nullable)
  // kStoreConvT2x2: Cout = N/4, out is [B, 2Ho, 2Wo, out_cs]
  // kStoreHeadIllu:
  const float* head_w;    // [32] 1x1 weights
  float head_b;
  const float* x_nchw;    // network input (fp32 or T per x_f16), [B,3,Ho,Wo]
  int x_f16;
  float* illu;            // [B,1,Ho,Wo] fp32 output (or T when illu_f16)
  int illu_f16;
  // second output (fp16, kStoreNHWC only; nullable): out2[m*out2_cs + n] =
  // relu(fma(o, pre2_scale[n], pre2_shift[n])) of the fp16-rounded stored value
  // o -- the next PreActResBlock's relu(bn1(x)) (models/model.py:164-166)
  // written by the producer's epilogue instead of a separate pass
  void* out2; int out2_cs;
  const float* pre2_scale;
  const float* pre2_shift;
  // fp32 output of an fp16 conv (the training step's autocast convs, nullable;
  // launch_conv_out32 only): out32[pix * out32_cs + out32_coff + n] =
  // (float)(fp16-rounded result) + res32[pix * res32_cs + n] (res32 nullable,
  // may alias out32); `out` is not written
  float* out32; int out32_cs, out32_coff;
  const float* res32; int res32_cs;
  // with out32 (nullable): a compact fp16 copy of the same outputs,
  // out32_h16[pix * out32_h16_cs + n] = (half)(the fp32 value stored) -- the
  // next autocast conv's operand, so it needs no cast pass of its own
  void* out32_h16; int out32_h16_cs;
  // with out32 (nullable): both outputs zeroed where mask16[pix * mask16_cs +
  // n] <= 0 -- the ReLU backward of the activation this input gradient flows
  // into, fused (mask16 = that activation's fp16 copy); skip32: out32 is not
  // written, only out32_h16 (a gradient whose one reader takes the fp16 copy)
  const void* mask16; int mask16_cs; int skip32;
  // with out32, a 1x1 stride-1 op over an H x W input (launch_conv_pw only):
  // input pixel (b, i, j) lands at output pixel (b, 2i, 2j) of a 2H x 2W map,
  // the others are not written (the 1x1 stride-2 conv's input gradient)
  int out_s2;
  // hwide4 pointwise form (its dispatcher sets 1, 0 elsewhere): each tile walks
  // its K chunks starting at chunk mtile % NCH instead of 0.  Always on where
  // it is read; the field stays because the kernel without the test of it
  // allocates 8 more VGPRs in the 4-chunk program (248 -> 256)
  int krot;
  // Split-fp16 form of an fp32 conv (launch_conv_wide only).  A split tensor
  // stores C fp32 channels per pixel as 2C fp16: [hi(C) | lo(C)], hi = (half)v,
  // lo = (half)((v - hi) * 2^11), v = hi + lo * 2^-11.  The segments and packed
  // weights carry the split operands (split_pack.hip pack_split); here only the
  // epilogue differs: every value is taken from the fp32 accumulator, never
  // from its fp16 rounding.
  // split_out (nullable): hi at split_out[pix * split_cs + ch], lo split_lo
  // halfs further (NHWC: split_lo = N, ConvT pixel shuffle: N / 4); `out` is
  // not written.  out_f32 (nullable): the plain fp32 value instead (NHWC).
  // split_res: res1 / res2 are split tensors (lo at + N).  ovf (nullable): set
  // to 1 with a plain store when a stored |v| > 65504 or v is not finite.
  void* split_out; int split_cs, split_lo;
  float* out_f32; int out_f32_cs;
  int split_res;
  // Split in registers (fp32 row ring only; 0 elsewhere):
  // tensors, DMA and LDS stay fp32, each 8-channel fragment is split into (hi,
  // lo) fp16 after its LDS read (split_f32x8) and the products run on the fp16
  // MFMA unit as hi W_hi + hi W_lo + (lo W_hi) 2^-11 with per-output-channel
  // power-of-two weight scales.  kMma16Offer: a kernel that does not take the
  // op in this form runs its exact fp32 form (launch_conv's `form` tells which
  // ran); kMma16Only: it answers kErrUnsupported instead (launch_conv_regs).
  // ovf as above: set when an accumulator is not finite (an input left the
  // fp16 range).  kMma16WSplit (launch_conv_wsplit only): the weights were
  // split once on the host -- W is the fp16 plane blob of split_pack.hip
  // pack_split_w ([N][Kpad / 32][W_hi(32) | W_lo(32)], as many bytes per row as
  // the fp32 weights), scale the 1 / s_n vector; only the activation fragments
  // are split in the kernel.
  // (placed in the padding before ovf: the struct, and with it every kernel
  // argument block, keeps its layout)
  int mma16;
  unsigned* ovf;
  // Where the row ring's split-in-registers programs (kMma16Offer / Only)
  // split their activations; every choice gives the same bits.
  // kRingSplitDefault: once per ring element, in LDS, in the form (Top or
  // Ahead) that measured faster for the program; kRingSplitTap: once per tap,
  // in registers after the LDS read; kRingSplitTop: in LDS at the top of the
  // step that first reads the group, behind a second barrier; kRingSplitAhead:
  // in LDS one step ahead of the first reader, beside the MFMAs, in a 5-group
  // ring.  (The switches that set this and w64_tile: split_pack.h.)
  int ring_split;
  // launch_conv_wsplit: 0 = the 64 -> 64 stride-1 3x3 programs run on the row
  // ring (conv_ring64.hip) and what it refuses on the gathered tile; 1 = the
  // tile kernel alone.  The ring's schedule follows ring_split (Top, Ahead,
  // else its default)
  int w64_tile;
};

// ConvOp::mma16
enum : int {
  kMma16Off = 0,
  kMma16Offer = 1,   // split in registers where a kernel has the form, else the exact program
  kMma16Only = 2,    // split in registers or kErrUnsupported
  kMma16WSplit = 3,  // weights split once on the host
};
// ConvOp::ring_split
enum : int { kRingSplitDefault = 0, kRingSplitTap = 1, kRingSplitTop = 2, kRingSplitAhead = 3 };
// The form an op ran in (upr_model_op_forms, include/upr.h UprOpForm::form)
enum : int {
  kFormExact = 0,   // the model dtype's own kernels
  kFormRegion = 1,  // split-fp16 region (ConvOp::split_out)
  kFormRegs = 2,    // split in registers
  kFormWSplit = 3,  // weights split once
};
// The kernel launch_conv_wsplit ran (upr_conv_wsplit_ran)
enum : int { kWSplitNone = 0, kWSplitTile = 1, kWSplitRing = 2 };

// 2^11 / 2^-11: the scale of the lo half of a split-fp16 value (ConvOp::split_out)
constexpr float kSplitLoScale = 2048.f;
constexpr float kSplitLoInv = 1.f / 2048.f;

#ifdef __HIPCC__
typedef _Float16 f16x8_t __attribute__((ext_vector_type(8)));
// 8 fp32 values -> split fp16: hi = (half)v, lo = (half)((v - hi) 2^11),
// plain round-to-nearest casts (fp16 subnormals kept).  |v| >= 65520 gives
// hi = +-inf and a non-finite lo: the caller's accumulators go non-finite.
__device__ __forceinline__ void split_f32x8(const float (&v)[8], f16x8_t& hi, f16x8_t& lo) {
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const half_t h = (half_t)v[i];
    hi[i] = h;
    lo[i] = (half_t)__builtin_fmaf((float)h, -kSplitLoScale, v[i] * kSplitLoScale);
  }
}
// weights: w s_n -> W_hi = (half)(w s), W_lo = (half)(w s - W_hi)
__device__ __forceinline__ void split_w_f32x8(const float (&v)[8], float s, f16x8_t& hi, f16x8_t& lo) {
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const float w = v[i] * s;
    const half_t h = (half_t)w;
    hi[i] = h;
    lo[i] = (half_t)(w - (float)h);
  }
}
#endif
// The exponent sh of the power of two s = 2^sh with max|w| s in [2^14, 2^15)
// for a weight row of largest magnitude mx (pack_split's rule: 0 for a zero or
// non-finite row, clamped to +-100); host and device
__host__ __device__ inline int split_row_shift(float mx) {
  int sh = 0;
  if (mx > 0.f && mx < __builtin_inff()) {
    int e;
    (void)__builtin_frexpf(mx, &e);
    sh = 15 - e;
    sh = sh < -100 ? -100 : sh > 100 ? 100 : sh;
  }
  return sh;
}

// fp32 NHWC [npix][C] <-> split fp16 [npix][2C] (C % 8 == 0; split_pack.hip)
int launch_split_f32(const float* x, void* y, size_t npix, int C, unsigned* ovf, hipStream_t st);
int launch_unsplit_f32(const void* x, float* y, size_t npix, int C, hipStream_t st);

// fp16 convs with an fp32 output (ConvOp::out32): the wide-tile and row-ring
// kernels; kErrUnsupported when neither takes the op
int launch_conv_out32(const ConvOp& op, hipStream_t stream);
// the input gradient of a 3x3 stride-2 pad-1 conv straight from dy (conv_pw.hip;
// op = the stride-1 dgrad op over dy with the flipped filter, output 2H x 2W)
int launch_conv_s2dg(const ConvOp& op, hipStream_t stream, bool probe = false);
// fp16 1x1 streaming convs (conv_pw.hip); probe: only answer kOk / kErrUnsupported
int launch_conv_pw(const ConvOp& op, hipStream_t stream, bool probe = false);

// form (nullable): the form the op ran in, kFormExact or kFormRegs (ConvOp::mma16)
int launch_conv(const ConvOp& op, int dtype, hipStream_t stream, int* form = nullptr);
// an fp32 op in the split-in-registers form only (sets mma16 = kMma16Only):
// kOk, or kErrUnsupported when no kernel takes it in that form
int launch_conv_regs(const ConvOp& op, hipStream_t stream, int* form = nullptr);

int launch_conv_ring32(const ConvOp& op, hipStream_t st, int* form = nullptr);
// an fp32 op with its weights split once (ConvOp::mma16 == kMma16WSplit;
// conv_wide32.hip): kOk, or kErrUnsupported -- it never runs another form.  Two
// kernels: the row ring for the ops launch_conv_ring_w64 takes (unless
// ConvOp::w64_tile), the gathered 256 x 64 tile for the rest; kernel
// (nullable): which one ran, kWSplitNone when the op was refused
int launch_conv_wsplit(const ConvOp& op, hipStream_t st, int* kernel = nullptr);
// the row-ring kernel of that form alone (conv_ring64.hip): kOk or kErrUnsupported
int launch_conv_ring_w64(const ConvOp& op, hipStream_t st);
// position of channel c (0..31) of a 32-deep K step within a 32-half weight
// plane of that form: lane group g = (c % 16) / 4 holds the 8 k-slots 4g..4g+3,
// 16+4g..16+4g+3, the channels of its two ds_read_b128 of an fp32 A row
inline int wsplit_kslot(int c) { return ((c & 15) >> 2) * 8 + (c >> 4) * 4 + (c & 3); }
// fp16 wide-tile convs (conv_wide.hip), also the split-fp16 form of fp32 convs
// (ConvOp::split_out); probe: only answer kOk / kErrUnsupported
int launch_conv_wide(const ConvOp& op, hipStream_t st, bool probe = false);

inline int cdiv(int a, int b) { return (a + b - 1) / b; }

// Per-(image, channel) pool sums (ConvOp::pool: EnhancedFAM channel attention,
// ASPP global branch) are accumulated as 64-bit fixed point (2^-24 units) with
// integer atomics: the sum no longer depends on the order in which tiles /
// units finish, so a forward is bit-for-bit reproducible.  A pool entry is 16
// bytes (the float* is only the carrier type): the int64 sum, then a uint32 of
// non-finite flags (bit 0 a +inf, bit 1 a -inf, bit 2 a NaN contribution),
// set with an atomic OR instead of converting the value, so pool_get returns
// what torch's mean would (+inf, -inf, or NaN for NaN / +inf with -inf).
constexpr float kPoolScale = 16777216.f;  // 2^24
constexpr int kPoolEntryFloats = 4;       // 16-byte entries
#ifdef __HIPCC__
__device__ __forceinline__ void pool_add(float* pool, size_t idx, float v) {
  if (__builtin_isfinite(v)) {
    atomicAdd((unsigned long long*)pool + 2 * idx, (unsigned long long)__float2ll_rn(v * kPoolScale));
  } else {
    const unsigned f = __builtin_isnan(v) ? 4u : (v > 0.f ? 1u : 2u);
    atomicOr((unsigned*)pool + 4 * idx + 2, f);
  }
}
__device__ __forceinline__ float pool_get(const float* pool, size_t idx) {
  const unsigned f = ((const unsigned*)pool)[4 * idx + 2];
  if (f) return (f & 4u) || (f & 3u) == 3u ? __builtin_nanf("") : ((f & 1u) ? __builtin_inff() : -__builtin_inff());
  return (float)((double)(long long)((const unsigned long long*)pool)[2 * idx] * (1.0 / 16777216.0));
}
#endif
inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// Per-(device, stream) scratch of the training kernels (split-K slabs,
// argmax codes, bilinear row sums, partial sums): one growable buffer per
// slot, reused by every later call on that stream -- the calls are
// stream-ordered, so a buffer is never live in two of them at once; buffers
// that ARE live together (a nested call) take different slots.  Replaces
// hipMallocAsync / hipFreeAsync, which cost 0.1-0.5 ms of host time per
// call on this stack (13 of 36 ms per training step went to them) and
// stalled the launch queue.  Growth (warm-up only) synchronises the stream
// before freeing the smaller buffer.  Returns nullptr when out of memory.
// At most kScratchStreams (device, stream) pairs hold buffers; a new pair past
// that reclaims the least recently used entry that only the calling thread
// ever used (after a device synchronise: that thread's earlier calls have all
// enqueued their launches), and gets nullptr (the caller's entry point returns
// an error) only when every entry is another thread's or shared, or while its
// stream is being captured.
constexpr int kScratchStreams = 64;
enum ScratchSlot { kSlotSlab = 0, kSlotCast, kSlotTmp, kSlotCode, kSlotRows, kSlotPart, kSlotMs, kSlotCount };
// fresh (optional): set true when the returned buffer was (re)allocated by this call
void* scratch(int slot, size_t bytes, hipStream_t st, bool* fresh = nullptr);

}  // namespace upr
