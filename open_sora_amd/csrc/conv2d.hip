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
// K runs tap-major / channel-minor (k = tap * Cin + ci), so every 16-byte chunk of the A tile is 8 contiguous channels of ONE
// input pixel: coalesced 16 B loads straight into LDS (global_load_lds_dwordx4), the lane-linear, source-swizzled LDS image of the
// dense GEMM (gemm_bf16.hip).  Tile 128 pixels x 128 Cout x 64 K, 4 waves (2 x 2) of 2 x 2 v_mfma_f32_32x32x16_bf16 tiles, operands
// swapped so an accumulator lane owns one output pixel and 4 consecutive channels: bias, residual and the bf16 pack are lane-local.
// The 128 pixels of a tile are an 8 x 16 spatial brick of one image (whole bricks: H % 8 == 0 and W % 16 == 0 at the output), so
// the 10 x 18 input pixels its 9 taps read are shared by the whole tile through L1 / L2; other sizes walk the pixels row-major.
//
// Roofline: MFMA bf16.  Algorithmic FLOPs = 2 * Cin * Cout * k^2 * B*Ho*Wo.
#include "osk_common.h"
#include "../../include/osk.h"

namespace {

constexpr int BM = 128, BN = 128, BK = 64;
constexpr int TILE_BYTES = 128 * BK * 2;
constexpr int SMEM_BYTES = 2 * 2 * TILE_BYTES;

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

OSK_DEV void glds16(const unsigned short* g, unsigned char* lds_wave_base) {
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)g,
                                   (__attribute__((address_space(3))) void*)lds_wave_base, 16, 0, 0);
}

// output pixel index (row-major b, ho, wo) of tile row r of tile bm
OSK_DEV int tile_pixel(const Conv2dParams& p, int bm, int r) {
  if (!p.brick) return bm * BM + r;
  const int bw = p.Wo >> 4, bh = p.Ho >> 3;
  const int bx = bm % bw;
  int q = bm / bw;
  const int by = q % bh;
  const int b = q / bh;
  return (b * p.Ho + by * 8 + (r >> 4)) * p.Wo + bx * 16 + (r & 15);
}

// BIGC: Cin % 64 == 0 -> a K tile lies inside one tap (tap is wave-uniform)
template <bool BIGC>
__global__ void __launch_bounds__(256, 2) conv2d_kernel(const Conv2dParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const int hi = lane >> 5, l31 = lane & 31;

  const int nbm = (p.M + BM - 1) / BM, nbn = (p.Cout + BN - 1) / BN;
  const int tile = xcd_remap(blockIdx.x, nbm * nbn);
  const int bm = tile / nbn, bn = tile - bm * nbn;
  const int n0 = bn * BN;

  // ---- staging rows of this lane: 4 row-blocks of 8 rows per wave per operand (as conv3d.hip)
  const int srow8 = lane >> 3, spos = lane & 7;
  const unsigned short* gw[4];
  int lds_off[4], cch[4];
  int pB[4], pH[4], pW[4];   // image base pixel, first tap row / column in the upsampled frame (may be < 0: zero padding)
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int rb = i * 4 + wave;
    const int r = rb * 8 + srow8;
    cch[i] = spos ^ ((r >> 1) & 7);  // source chunk that must land at LDS position spos
    lds_off[i] = rb * 1024;
    int n = n0 + r;
    n = n < p.Cout ? n : p.Cout - 1;
    gw[i] = p.w + (int64_t)n * p.wrs + cch[i] * 8;
    int m = bm * BM + r < p.M ? tile_pixel(p, bm, r) : p.M - 1;   // tail rows re-read the last pixel (never stored)
    const int wo = m % p.Wo;
    const int q = m / p.Wo;
    const int ho = q % p.Ho;
    const int b = q / p.Ho;
    pB[i] = b * p.H * p.W;
    pH[i] = ho * p.st - p.pad;
    pW[i] = wo * p.st - p.pad;
  }

  f32x16_t acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  const int cpt_mask = (1 << p.lg_cpt) - 1;
  const int sw = (l31 >> 1) & 7;
  const int a_row_off = (wm * 64 + l31) * 128;
  const int w_row_off = (wn * 64 + l31) * 128;
  const int ush = p.up;

#define STAGE_ISSUE(BUFI, KT)                                                                     \
  {                                                                                               \
    unsigned char* ta_ = smem + (BUFI) * 2 * TILE_BYTES;                                          \
    unsigned char* tw_ = ta_ + TILE_BYTES;                                                        \
    int tap_u_ = 0, cc_u_ = 0;                                                                    \
    if constexpr (BIGC) {                                                                         \
      const int q_ = (KT) * 8;                                                                    \
      tap_u_ = q_ >> p.lg_cpt;                                                                    \
      cc_u_ = q_ & cpt_mask;                                                                      \
    }                                                                                             \
    _Pragma("unroll") for (int i = 0; i < 4; ++i) {                                               \
      int tap_, cc_;                                                                              \
      if constexpr (BIGC) {                                                                       \
        tap_ = tap_u_; cc_ = cc_u_ + cch[i];                                                      \
      } else {                                                                                    \
        const int q_ = (KT) * 8 + cch[i];                                                         \
        tap_ = q_ >> p.lg_cpt;                                                                    \
        cc_ = q_ & cpt_mask;                                                                      \
      }                                                                                           \
      const int dh_ = p.ks == 3 ? tap_ / 3 : 0;                                                   \
      const int dw_ = p.ks == 3 ? tap_ - dh_ * 3 : 0;                                             \
      const int hu_ = pH[i] + dh_, wu_ = pW[i] + dw_;                                             \
      const bool in_ = tap_ < p.ntaps && (unsigned)hu_ < (unsigned)p.Hu && (unsigned)wu_ < (unsigned)p.Wu; \
      const int pos_ = pB[i] + (hu_ >> ush) * p.W + (wu_ >> ush);                                 \
      const unsigned short* ga_ = in_ ? p.x + (((int64_t)pos_ << p.lg_cpt) + cc_) * 8 : conv2d_zero_page; \
      glds16(ga_, ta_ + lds_off[i]);                                                              \
    }                                                                                             \
    _Pragma("unroll") for (int i = 0; i < 4; ++i) glds16(gw[i] + (KT) * BK, tw_ + lds_off[i]);    \
  }

  STAGE_ISSUE(0, 0);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  int cur = 0;
  for (int kt = 0; kt < p.nk; ++kt) {
    const bool more = kt + 1 < p.nk;
    if (more) STAGE_ISSUE(cur ^ 1, kt + 1);
    const unsigned char* ta = smem + cur * 2 * TILE_BYTES;
    const unsigned char* tw = ta + TILE_BYTES;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      const int coff = (((ks << 1) | hi) ^ sw) << 4;
      bf16x8_t af[2], wf[2];
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        af[t] = *reinterpret_cast<const bf16x8_t*>(ta + a_row_off + t * 32 * 128 + coff);
        wf[t] = *reinterpret_cast<const bf16x8_t*>(tw + w_row_off + t * 32 * 128 + coff);
      }
#pragma unroll
      for (int tn = 0; tn < 2; ++tn)
#pragma unroll
        for (int tm = 0; tm < 2; ++tm)
          acc[tn][tm] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf[tn], af[tm], acc[tn][tm], 0, 0, 0);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    cur ^= 1;
  }
#undef STAGE_ISSUE

  // ---- epilogue: lane owns pixel m, channels n = quad*8 + hi*4 + {0..3}
  const bool vec_ok = (p.Cout & 3) == 0;
#pragma unroll
  for (int tm = 0; tm < 2; ++tm) {
    const int r = wm * 64 + tm * 32 + l31;
    if (bm * BM + r >= p.M) continue;
    const int m = tile_pixel(p, bm, r);
    const int64_t roff = (int64_t)m * p.Cout;
#pragma unroll
    for (int tn = 0; tn < 2; ++tn) {
#pragma unroll
      for (int qd = 0; qd < 4; ++qd) {
        const int n = n0 + wn * 64 + tn * 32 + qd * 8 + hi * 4;
        if (n >= p.Cout) continue;
        float v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = acc[tn][tm][qd * 4 + j];
        if (vec_ok && n + 3 < p.Cout) {
          if (p.bias) {
            const float4 bv = *reinterpret_cast<const float4*>(p.bias + n);
            v[0] += bv.x; v[1] += bv.y; v[2] += bv.z; v[3] += bv.w;
          }
          if (p.res) {
            const uint2 rv = *reinterpret_cast<const uint2*>(p.res + roff + n);
            v[0] += bf16_lo(rv.x); v[1] += bf16_hi(rv.x); v[2] += bf16_lo(rv.y); v[3] += bf16_hi(rv.y);
          }
          uint2 o;
          o.x = pack_bf16x2(v[0], v[1]);
          o.y = pack_bf16x2(v[2], v[3]);
          *reinterpret_cast<uint2*>(p.out + roff + n) = o;
        } else {
          for (int j = 0; j < 4 && n + j < p.Cout; ++j) {
            float t = v[j] + (p.bias ? p.bias[n + j] : 0.f);
            if (p.res) t += bf16_bits_to_f32(p.res[roff + n + j]);
            p.out[roff + n + j] = f32_to_bf16_bits(t);
          }
        }
      }
    }
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
  int lg = 0;
  while ((8 << lg) < Cin) ++lg;
  p.lg_cpt = lg;
  p.ntaps = ksize * ksize;
  const int64_t K = (int64_t)p.ntaps * Cin;
  const int64_t Kp = (K + BK - 1) / BK * BK;
  if (w_row_stride < Kp || (w_row_stride & 7)) return OSK_EINVAL;  // weight rows zero-padded to a multiple of 64
  p.wrs = w_row_stride;
  p.nk = (int)(Kp / BK);
  hipStream_t s = (hipStream_t)stream;
  const int nblk = ((p.M + BM - 1) / BM) * ((Cout + BN - 1) / BN);
  dim3 grid(nblk), block(256);
  if (Cin % 64 == 0) hipLaunchKernelGGL((conv2d_kernel<true>), grid, block, SMEM_BYTES, s, p);
  else hipLaunchKernelGGL((conv2d_kernel<false>), grid, block, SMEM_BYTES, s, p);
  return (int)hipGetLastError();
}
