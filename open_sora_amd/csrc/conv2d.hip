// Zero-padded 2-D convolution for gfx950 (the Flux image autoencoder) as an im2col-free implicit GEMM on MFMA bf16, NHWC
// activations.
//
//   out[b, ho, wo, co] = bias[co] + res[b, ho, wo, co] +
//        sum_{dh,dw,ci}  X[b, ho*stride + dh - pad, wo*stride + dw - pad, ci] * w[co, (dh*k + dw)*Cin + ci]
//
// X is the source seen through an optional nearest 2x upsample (Upsample, autoencoder_2d.py:115-122) and is ZERO outside the
// (upsampled) image: nn.Conv2d(padding=1) for pad = 1, the explicit (0, 1, 0, 1) zero pad of Downsample (autoencoder_2d.py:104-113)
// for pad = 0, stride 2.  Neither the padded nor the upsampled copy exists: the upsample is a shift of the gathered coordinate and an
// out-of-image tap row is loaded from a 16-byte page of zeros instead of the activation tensor.
//
// The tile is tile128.h's (128 pixels x 128 Cout x 64 K, its staging, LDS layout, K loop, epilogue and 8 x 16 brick order); what
// is this file's is the gather: the source address of (pixel, tap), or the page of zeros.
//
// Roofline: MFMA bf16.  Algorithmic FLOPs = 2 * Cin * Cout * k^2 * B*Ho*Wo.
#include "tile128.h"
#include "../../include/osk.h"

namespace {

using namespace osk_tile128;

// the source of every out-of-image (zero padding) or K-padding A-tile chunk
__device__ __attribute__((aligned(16))) unsigned short conv2d_zero_page[8];

struct Conv2dParams {
  const unsigned short* x;
  const unsigned short* w;
  const float* bias;
  const unsigned short* res;
  unsigned short* out;
  int B, H, W;       // source (pre-upsample) dims
  int Hu, Wu;        // dims the conv sees (after the virtual nearest upsample)
  int Ho, Wo;
  int Cin, Cout;
  int ks, st, pad, up;
  int lg_cpt, ntaps, nk;
  int M;
  int brick;         // 1 = a tile is an 8 x 16 brick of one image
  int64_t wrs;
};

// A operand: the 8-channel chunk of (pixel of staging row i, tap), from the image or from the zero page
template <bool BIGC>
struct Conv2dASrc {
  const Conv2dParams& p;
  int pB[4], pH[4], pW[4];   // image base pixel, first tap row / column in the upsampled frame (may be < 0: zero padding)
  __device__ __forceinline__ const unsigned short* operator()(const Lane& g, int i, int kt) const {
    const TapChunk tc = tap_chunk<BIGC>(kt, g.cch[i], p.lg_cpt);
    const int dh = p.ks == 3 ? tc.tap / 3 : 0;
    const int dw = p.ks == 3 ? tc.tap - dh * 3 : 0;
    const int hu = pH[i] + dh, wu = pW[i] + dw;
    const bool in = tc.tap < p.ntaps && (unsigned)hu < (unsigned)p.Hu && (unsigned)wu < (unsigned)p.Wu;
    const int pos = pB[i] + (hu >> p.up) * p.W + (wu >> p.up);
    return in ? p.x + (((int64_t)pos << p.lg_cpt) + tc.cc) * 8 : conv2d_zero_page;
  }
};

template <bool BIGC>
__global__ void __launch_bounds__(256, 2) conv2d_kernel(const Conv2dParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const Lane g = make_lane(p.M, p.Cout, p.w, p.wrs);

  Conv2dASrc<BIGC> a_src = {p};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    // tail rows re-read the last pixel (never stored)
    const int m = g.bm * BM + g.row[i] < p.M ? tile_row_index(p.brick, g.bm, g.row[i], p.Ho, p.Wo) : p.M - 1;
    const int wo = m % p.Wo;
    const int q = m / p.Wo;
    const int ho = q % p.Ho;
    const int b = q / p.Ho;
    a_src.pB[i] = b * p.H * p.W;
    a_src.pH[i] = ho * p.st - p.pad;
    a_src.pW[i] = wo * p.st - p.pad;
  }

  f32x16_t acc[2][2];
  mainloop(g, smem, p.nk, a_src, acc);

#pragma unroll
  for (int tm = 0; tm < 2; ++tm) {
    const int r = acc_row(g, tm);
    if (g.bm * BM + r >= p.M) continue;
    const int64_t roff = (int64_t)tile_row_index(p.brick, g.bm, r, p.Ho, p.Wo) * p.Cout;
    conv_epilogue_row(g, acc, tm, roff, p.Cout, p.bias, false, p.res, p.out);
  }
}

}  // namespace

extern "C" int osk_conv2d_nhwc_bf16(const void* x, int B, int H, int W, int Cin, const void* w, int64_t w_row_stride,
                                    const float* bias, int Cout, int ksize, int stride, int pad, int up, const void* res,
                                    void* out, int Ho, int Wo, double* gn_sums, int gn_groups, void* stream) {
  if (!x || !w || !out || B <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0 || Ho <= 0 || Wo <= 0) return OSK_EINVAL;
  if (ksize != 1 && ksize != 3) return OSK_EINVAL;
  if (stride != 1 && stride != 2) return OSK_EINVAL;
  if (pad < 0 || pad > ksize - 1 || (up != 0 && up != 1)) return OSK_EINVAL;
  if ((Cin & 7) || (Cin & (Cin - 1))) return OSK_EINVAL;  // Cin = 8 * 2^j (pad 3 -> 8 at the boundary)
  if (((uintptr_t)x & 15) || ((uintptr_t)w & 15) || ((uintptr_t)bias & 15) || ((uintptr_t)out & 7) || ((uintptr_t)res & 7))
    return OSK_EINVAL;
  if (gn_sums) {   // the fused-statistics epilogue is not built for this kernel: nothing is launched
    if (gn_groups <= 0 || ((uintptr_t)gn_sums & 7)) return OSK_EINVAL;
    return OSK_EUNSUPPORTED;
  }
  Conv2dParams p;
  p.x = (const unsigned short*)x; p.w = (const unsigned short*)w; p.bias = bias;
  p.res = (const unsigned short*)res; p.out = (unsigned short*)out;
  p.B = B; p.H = H; p.W = W; p.Cin = Cin; p.Cout = Cout;
  p.up = up;
  p.Hu = up ? 2 * H : H;
  p.Wu = up ? 2 * W : W;
  p.ks = ksize; p.st = stride; p.pad = pad;
  // every output window starts inside the padded frame: its first tap row / column is at most the last image row / column
  if ((int64_t)(Ho - 1) * stride - pad > p.Hu - 1 || (int64_t)(Wo - 1) * stride - pad > p.Wu - 1) return OSK_EINVAL;
  p.Ho = Ho; p.Wo = Wo;
  const int64_t M = (int64_t)B * Ho * Wo;
  if (M >= (int64_t)1 << 31 || (int64_t)B * H * W * Cin >= (int64_t)1 << 34) return OSK_EUNSUPPORTED;
  p.M = (int)M;
  p.brick = (Ho % 8 == 0 && Wo % 16 == 0) ? 1 : 0;
  p.ntaps = ksize * ksize;
  if (conv_k_layout(Cin, p.ntaps, w_row_stride, &p.lg_cpt, &p.nk) != OSK_OK) return OSK_EINVAL;
  p.wrs = w_row_stride;
  hipStream_t s = (hipStream_t)stream;
  const int nblk = ((p.M + BM - 1) / BM) * ((Cout + BN - 1) / BN);
  dim3 grid(nblk), block(256);
  if (Cin % 64 == 0) hipLaunchKernelGGL((conv2d_kernel<true>), grid, block, SMEM_BYTES, s, p);
  else hipLaunchKernelGGL((conv2d_kernel<false>), grid, block, SMEM_BYTES, s, p);
  return (int)hipGetLastError();
}
