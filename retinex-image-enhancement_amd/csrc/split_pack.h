// The split forms of the fp32 forward, host side: the two weight formats
// (split_pack.hip), the types the packers share with the graph builder
// (model.hip) and the op-level entry points (conv_api.hip), and the one reader
// of the environment switches that select a form.
#pragma once
#include <vector>

#include "upr_common.h"

namespace upr {

struct SegSpec {
  int src;       // buffer id
  int C, coff, cs;
  int kh, kw, stride, pad, dil;
  int pre;
  size_t pre_scale = 0, pre_shift = 0;  // float offsets (bytes) in blob
  int kbase;
};

inline SegSpec seg(int src, int C, int cs, int coff, int k, int stride, int pad, int dil, int pre = kPreNone) {
  SegSpec s;
  s.src = src; s.C = C; s.cs = cs; s.coff = coff;
  s.kh = k; s.kw = k; s.stride = stride; s.pad = pad; s.dil = dil;
  s.pre = pre; s.kbase = 0;
  return s;
}

// A K-segment's weights before packing: w[n][c][r][s] (row-major), already
// multiplied by any per-output-channel fold.
struct SegWeights {
  SegSpec spec;
  std::vector<double> w;  // N * C * kh * kw
};

// Split-fp16 form of an fp32 GEMM (pack_split, split_pack.hip)
struct SplitPack {
  int N = 0, Kpad = 0;
  std::vector<_Float16> W;     // [N][Kpad]
  std::vector<float> scale;    // [N]
  std::vector<SegSpec> segs;   // 2 per logical segment
};
// segs: plain segments (coff 0, cs == C, C % 64 == 0, no prologue); false otherwise
bool pack_split(int N, const std::vector<SegWeights>& segs, SplitPack& out);

// Weights split once (pack_split_w, split_pack.hip)
struct SplitWPack {
  std::vector<_Float16> W;   // [N][K / 32][2][32]
  std::vector<float> scale;  // [N]
};
bool pack_split_w(int N, int K, const float* w, SplitWPack& out);
// bytes of upr_pack_split_w_f32's blob: the planes (4 bytes per weight), then 1 / s_n
size_t split_w_bytes(int Cout, int K, size_t* scale_off);

// The environment switches of the split forms, as they are set when
// read_split_switches is called: upr_model_create reads them once per handle,
// the op-level entry points (conv_api.hip) at every call.  The value mappings
// are stated in read_split_switches and nowhere else (INTEGRATION.md has the
// table).
struct SplitSwitches {
  bool region;     // the split-fp16 region of the plain fp32 graph (form 1)
  bool regs;       // split in registers on the 32-channel row ring (form 2)
  bool w64;        // weights split once for the 64-wide convs (form 3)
  int ring_split;  // ConvOp::ring_split of the form 2 / 3 ring programs
  int w64_tile;    // ConvOp::w64_tile of the form 3 ops
};
SplitSwitches read_split_switches();
extern const char kSwitchRegion[];  // the name of the switch behind SplitSwitches::region, for messages

}  // namespace upr
