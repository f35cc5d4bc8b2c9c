// Launch parameters shared by the CausalConv3d kernels (conv3d.hip, conv3d_256.hip).
#pragma once
#include "osk_common.h"

namespace osk_conv {

struct ConvParams {
  const unsigned short* x;
  const unsigned short* w;
  const float* bias;
  const unsigned short* res;
  unsigned short* out;
  int B, T, H, W;     // source (pre-upsample) dims
  int Tu, Hu, Wu;     // dims the conv sees (after the virtual nearest upsample)
  int To, Ho, Wo;
  int Cin, Cout;
  int ks, st, sh, sw, up_t, up_hw;
  int lg_cpt, ntaps, nk;
  int M;
  int64_t wrs;
  int brick = 0;      // 1 = a tile is a 16 x 16 spatial brick of one frame, tiles ordered frame-fastest (conv3d_256.hip)
  // fused GroupNorm statistics of the OUTPUT (conv3d_256.hip only): sums[b][g] += (sum y, sum y^2) over the bf16-rounded
  // outputs of group g (gn_G groups of Cout / gn_G adjacent channels); null = off
  double* gn_sums = nullptr;
  int gn_G = 0;
  // GroupNorm + SiLU of the INPUT folded into the halo refill (conv3d_256.hip, sliding-window kernels, plain geometry): the conv
  // sees bf16(silu(bf16(x a + d))); table f32 [B][Cin / 8][16] = 8 scales a then 8 shifts d per 8-channel chunk
  // (osk_groupnorm_table_f32); null = the input as stored
  const float* gn_in = nullptr;
};


// The kernel that serves a call (values = OSK_CONV_* of include/osk.h, which osk_causal_conv3d_kernel_class reports)
enum ConvKernelClass : int {
  CONV_TILE128 = 0,        // conv3d_kernel<false>: the 128 x 128 implicit-GEMM tile, Cin % 64 != 0
  CONV_TILE128_BIGC = 1,   // conv3d_kernel<true>: the same tile, whole 64-channel K steps per tap
  CONV_FEWOUT = 2,         // conv_fewout_kernel<Cout>
  CONV_X4 = 3,             // conv256x_kernel<4>
  CONV_X8 = 4,             // conv256x_kernel<8>
  CONV_SW4 = 5,            // convsw_kernel<4, false>
  CONV_SW8 = 6,            // convsw_kernel<8, false>
  CONV_SW4_UP = 7,         // convsw_kernel<4, true>
  CONV_SW8_UP = 8,         // convsw_kernel<8, true>
  CONV_SW8_GN = 9,         // convsw_kernel<8, false, true>
  CONV_SW2 = 10,           // convsw2_kernel<false>
  CONV_SW2_GN = 11,        // convsw2_kernel<true>
};
struct ConvChoice {
  ConvKernelClass cls;
  bool stats;              // the fused-statistics epilogue is on
};

// conv3d_256.hip: 256 voxels x {256,128} channels x 64 tile, 4 waves, all 27 taps in one hand-scheduled asm K loop
bool conv256_supported(const ConvParams& p, int64_t x_bytes, int64_t w_bytes);
bool conv256_gn_supported(const ConvParams& p);   // the fused-statistics epilogue takes this output geometry
bool conv256_gn_in_supported(const ConvParams& p);   // a kernel with the input GroupNorm + SiLU folded in takes this shape
// THE selection: the kernel that serves p (geometry filled in; of x / w / bias / res / out / gn_sums / gn_in only null-ness and
// alignment are looked at, nothing is dereferenced) -> OSK_OK and *c, or OSK_EUNSUPPORTED where gn_sums / gn_in was asked of a
// shape whose kernel does not carry it (nothing may be launched then).  conv_entry launches by switching on *c.
int conv_kernel_class(const ConvParams& p, ConvChoice* c);
int launch_conv256(const ConvParams& p, ConvKernelClass cls, hipStream_t st);

}  // namespace osk_conv
