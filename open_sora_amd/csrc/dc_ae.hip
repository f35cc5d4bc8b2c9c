// Kernels of the Video DC-AE autoencoder (dc-ae-f32t4c128) for gfx950: every operator of
// opensora/models/dc_ae/models/nn/ops.py the decoder and the encoder run, on channels-last NDHWC bf16 activations.
//
//   osk_conv3d_zp_ndhwc_bf16     ConvLayer(is_video) k = 1 / 3: zero "same" padding on all six faces, + nearest upsample in front
//                                (T and H,W independently), + bias, + SiLU, + residual add behind.  MFMA implicit GEMM.
//   osk_conv3d_zp_strided_ndhwc_bf16  the encoder's downsample ConvLayer: k = 3, stride (1|2, 2, 2), zero padding 1, + bias,
//                                + residual add.  The same tile; the gathered coordinate is out * stride - 1 + tap.
//   osk_dup_shuffle_ndhwc_bf16   ChannelDuplicatingPixelShuffleUpSampleLayer: a pure gather (repeat_interleave + pixel shuffle).
//   osk_unshuffle_avg_ndhwc_bf16 PixelUnshuffleChannelAveragingDownSampleLayer: pixel unshuffle + mean over channel groups.
//   osk_dwconv3d_ndhwc_bf16      depthwise Conv3d k = 3 / 5, zero padded, + bias, + the GLU x * silu(gate) of GLUMBConv.
//   osk_gconv32_bf16             block-diagonal 1x1x1 conv, 32 -> 32 channels per group (LiteMLA.aggreg[0][1]).  MFMA.
//   osk_relu_linear_attn_bf16    LiteMLA.relu_linear_att per (batch, 96-channel [q|k|v] group), f32 accumulation.
//   osk_rmsnorm_affine_bf16      RMSNorm3d over channels with weight and bias, + ReLU, + identity-shortcut add.
//
// The convolution runs on tile128.h's tile (128 voxels x 128 Cout x 64 K, its staging, LDS layout, K loop, epilogue and 8 x 16 brick
// order of one frame); what is this file's is the gather: an out-of-volume tap is loaded from a 16-byte page of zeros, the upsample
// is a shift of the gathered coordinate.  Cout = 3 (project_out) runs on the same tile with 3 live columns: one code path, at the
// price of a 128 -> 128 conv.
//
// Roofline: conv MFMA bf16 (2 * Cin * Cout * k^3 * voxels FLOPs); everything else HBM / L2 bound.
#include "tile128.h"
#include "../../include/osk.h"

namespace {

using namespace osk_tile128;

// the source of every out-of-volume (zero padding) or K-padding A-tile chunk
__device__ __attribute__((aligned(16))) unsigned short conv3d_zero_page[8];

struct Conv3dParams {
  const unsigned short* x;
  const unsigned short* w;
  const float* bias;
  const unsigned short* res;
  unsigned short* out;
  int T, H, W;       // source (pre-upsample / pre-stride) dims
  int Tu, Hu, Wu;    // output dims (stride 1: also the dims the conv sees)
  int Cout;
  int ks, ut, uh, act;
  int st, sh;        // strided conv only: temporal and spatial stride
  int lg_cpt, ntaps, nk;
  int M;
  int brick;         // 1 = a tile is an 8 x 16 brick of one frame
  int64_t wrs;
};

// A operand: the 8-channel chunk of (voxel of staging row i, tap), from the volume or from the zero page
template <bool BIGC>
struct Conv3dASrc {
  const Conv3dParams& p;
  int pB[4], pT[4], pH[4], pW[4];   // batch base frame, first tap coordinate in the upsampled volume (may be < 0: zero padding)
  __device__ __forceinline__ void set(int i, int b, int to, int ho, int wo) {
    const int pad = p.ks >> 1;
    pB[i] = b * p.T;
    pT[i] = to - pad;
    pH[i] = ho - pad;
    pW[i] = wo - pad;
  }
  __device__ __forceinline__ const unsigned short* operator()(const Lane& g, int i, int kt) const {
    const TapChunk tc = tap_chunk<BIGC>(kt, g.cch[i], p.lg_cpt);
    const Tap3 d = tap3(tc.tap, p.ks);
    const int tu = pT[i] + d.dt, hu = pH[i] + d.dh, wu = pW[i] + d.dw;
    const bool in = tc.tap < p.ntaps && (unsigned)tu < (unsigned)p.Tu && (unsigned)hu < (unsigned)p.Hu && (unsigned)wu < (unsigned)p.Wu;
    const int pos = ((pB[i] + (tu >> p.ut)) * p.H + (hu >> p.uh)) * p.W + (wu >> p.uh);
    return in ? p.x + (((int64_t)pos << p.lg_cpt) + tc.cc) * 8 : conv3d_zero_page;
  }
};

// A operand of the strided conv (k = 3, padding 1): the first tap of output (to, ho, wo) sits at source (to * st - 1, ho * sh - 1,
// wo * sh - 1).  The batch base stays apart from the temporal coordinate, so a padded tap of batch b is a zero, never batch b +- 1
template <bool BIGC>
struct Conv3dStridedASrc {
  const Conv3dParams& p;
  int pB[4], pT[4], pH[4], pW[4];   // batch base frame, first tap coordinate in the source volume (-1: zero padding)
  __device__ __forceinline__ void set(int i, int b, int to, int ho, int wo) {
    pB[i] = b * p.T;
    pT[i] = to * p.st - 1;
    pH[i] = ho * p.sh - 1;
    pW[i] = wo * p.sh - 1;
  }
  __device__ __forceinline__ const unsigned short* operator()(const Lane& g, int i, int kt) const {
    const TapChunk tc = tap_chunk<BIGC>(kt, g.cch[i], p.lg_cpt);
    const Tap3 d = tap3(tc.tap, 3);
    const int t = pT[i] + d.dt, h = pH[i] + d.dh, w = pW[i] + d.dw;
    const bool in = tc.tap < p.ntaps && (unsigned)t < (unsigned)p.T && (unsigned)h < (unsigned)p.H && (unsigned)w < (unsigned)p.W;
    const int pos = ((pB[i] + t) * p.H + h) * p.W + w;
    return in ? p.x + (((int64_t)pos << p.lg_cpt) + tc.cc) * 8 : conv3d_zero_page;
  }
};

template <class ASrc>
__global__ void __launch_bounds__(256, 2) conv3d_zp_kernel(const Conv3dParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const Lane g = make_lane(p.M, p.Cout, p.w, p.wrs);

  ASrc a_src = {p};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    // tail rows re-read the last voxel (never stored)
    const int m = g.bm * BM + g.row[i] < p.M ? tile_row_index(p.brick, g.bm, g.row[i], p.Hu, p.Wu) : p.M - 1;
    const int wo = m % p.Wu;
    int q = m / p.Wu;
    const int ho = q % p.Hu;
    q /= p.Hu;
    const int to = q % p.Tu;
    const int b = q / p.Tu;
    a_src.set(i, b, to, ho, wo);
  }

  f32x16_t acc[2][2];
  mainloop(g, smem, p.nk, a_src, acc);

#pragma unroll
  for (int tm = 0; tm < 2; ++tm) {
    const int r = acc_row(g, tm);
    if (g.bm * BM + r >= p.M) continue;
    const int64_t roff = (int64_t)tile_row_index(p.brick, g.bm, r, p.Hu, p.Wu) * p.Cout;
    conv_epilogue_row(g, acc, tm, roff, p.Cout, p.bias, p.act, p.res, p.out);
  }
}

// ---------------------------------------------------------------------------------------------------------------------------
// out[b, to, ho, wo, co] = x[b, to / ft, ho / fh, wo / fh, (((co * ft + to % ft) * fh + ho % fh) * fh + wo % fh) / rep]
// one thread = 8 output channels of one output voxel
__global__ void __launch_bounds__(256) dup_shuffle_kernel(const unsigned short* __restrict__ x, unsigned short* __restrict__ out,
                                                          int T, int H, int W, int Cin, int Cout, int ft, int fh, int rep,
                                                          int64_t total) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int cchunks = Cout >> 3;
  const int c0 = (int)(idx % cchunks) * 8;
  int64_t v = idx / cchunks;
  const int Wo = W * fh, Ho = H * fh, To = T * ft;
  const int wo = (int)(v % Wo); v /= Wo;
  const int ho = (int)(v % Ho); v /= Ho;
  const int to = (int)(v % To);
  const int b = (int)(v / To);
  const int64_t src = ((((int64_t)b * T + to / ft) * H + ho / fh) * W + wo / fh) * Cin;
  const int sub = ((to % ft) * fh + ho % fh) * fh + wo % fh;
  const int per = ft * fh * fh;
  unsigned short r[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) r[j] = x[src + ((c0 + j) * per + sub) / rep];
  uint4 o;
  o.x = r[0] | ((unsigned)r[1] << 16);
  o.y = r[2] | ((unsigned)r[3] << 16);
  o.z = r[4] | ((unsigned)r[5] << 16);
  o.w = r[6] | ((unsigned)r[7] << 16);
  *reinterpret_cast<uint4*>(out + idx * 8) = o;
}

// ---------------------------------------------------------------------------------------------------------------------------
// out[b, t, h, w, co] = mean over g < gs of x[b, t*ft + dt, h*fh + dh, w*fh + dw, c],  u = co*gs + g, c = u / per, s = u % per,
// (dt, dh, dw) = (s / fh^2, (s / fh) % fh, s % fh), per = ft * fh^2.  One thread = 8 output channels of one output voxel: the
// 8 * gs consecutive u it sums walk the sub-voxels fastest and the source channels slowest
__global__ void __launch_bounds__(256) unshuffle_avg_kernel(const unsigned short* __restrict__ x, unsigned short* __restrict__ out,
                                                            int To, int Ho, int Wo, int Cin, int Cout, int ft, int fh, int gs,
                                                            float inv_gs, int64_t total) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int cchunks = Cout >> 3;
  const int c0 = (int)(idx % cchunks) * 8;
  int64_t v = idx / cchunks;
  const int wo = (int)(v % Wo); v /= Wo;
  const int ho = (int)(v % Ho); v /= Ho;
  const int to = (int)(v % To);
  const int b = (int)(v / To);
  const int H = Ho * fh, W = Wo * fh;
  const int fh2 = fh * fh, per = ft * fh2;
  const int64_t src = ((((int64_t)b * To + to) * ft * H + (int64_t)ho * fh) * W + (int64_t)wo * fh) * Cin;
  float a[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    float t = 0.f;
    for (int k = 0; k < gs; ++k) {
      const int u = (c0 + j) * gs + k;
      const int c = u / per, s = u - c * per;
      const int dt = s / fh2, dh = (s / fh) % fh, dw = s % fh;
      t += bf16_bits_to_f32(x[src + ((int64_t)(dt * H + dh) * W + dw) * Cin + c]);
    }
    a[j] = t * inv_gs;
  }
  *reinterpret_cast<uint4*>(out + idx * 8) = pack8(a);
}

// ---------------------------------------------------------------------------------------------------------------------------
// depthwise conv: one thread = 8 output channels of one voxel.  GLU: out[c] = (y[c] + b[c]) * silu(y[c + Co] + b[c + Co])
template <int KS, bool GLU>
__global__ void __launch_bounds__(256) dwconv3d_kernel(const unsigned short* __restrict__ x, const unsigned short* __restrict__ w,
                                                       const float* __restrict__ bias, unsigned short* __restrict__ out,
                                                       int T, int H, int W, int C, int64_t total) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int Co = GLU ? C >> 1 : C;
  const int cchunks = Co >> 3;
  const int c0 = (int)(idx % cchunks) * 8;
  int64_t v = idx / cchunks;
  const int wo = (int)(v % W); v /= W;
  const int ho = (int)(v % H); v /= H;
  const int to = (int)(v % T);
  const int b = (int)(v / T);
  constexpr int P = KS / 2;
  float a0[8], a1[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) { a0[j] = 0.f; a1[j] = 0.f; }
  for (int dt = 0; dt < KS; ++dt) {
    const int t = to + dt - P;
    if ((unsigned)t >= (unsigned)T) continue;
    for (int dh = 0; dh < KS; ++dh) {
      const int h = ho + dh - P;
      if ((unsigned)h >= (unsigned)H) continue;
#pragma unroll
      for (int dw = 0; dw < KS; ++dw) {
        const int ww = wo + dw - P;
        if ((unsigned)ww >= (unsigned)W) continue;
        const int64_t xo = ((((int64_t)b * T + t) * H + h) * W + ww) * C + c0;
        const int64_t wo_ = (int64_t)((dt * KS + dh) * KS + dw) * C + c0;
        float xf[8], wf[8];
        unpack8(*reinterpret_cast<const uint4*>(x + xo), xf);
        unpack8(*reinterpret_cast<const uint4*>(w + wo_), wf);
#pragma unroll
        for (int j = 0; j < 8; ++j) a0[j] = __builtin_fmaf(xf[j], wf[j], a0[j]);
        if constexpr (GLU) {
          unpack8(*reinterpret_cast<const uint4*>(x + xo + Co), xf);
          unpack8(*reinterpret_cast<const uint4*>(w + wo_ + Co), wf);
#pragma unroll
          for (int j = 0; j < 8; ++j) a1[j] = __builtin_fmaf(xf[j], wf[j], a1[j]);
        }
      }
    }
  }
  if (bias) {
#pragma unroll
    for (int j = 0; j < 8; ++j) a0[j] += bias[c0 + j];
    if constexpr (GLU) {
#pragma unroll
      for (int j = 0; j < 8; ++j) a1[j] += bias[c0 + Co + j];
    }
  }
  if constexpr (GLU) {
#pragma unroll
    for (int j = 0; j < 8; ++j) a0[j] *= silu(a1[j]);
  }
  *reinterpret_cast<uint4*>(out + idx * 8) = pack8(a0);
}

// ---------------------------------------------------------------------------------------------------------------------------
// block-diagonal 1x1x1 conv, 32 -> 32 per group: one wave = 32 tokens x one group, two 32x32x16 MFMAs, operands from global
__global__ void __launch_bounds__(256) gconv32_kernel(const unsigned short* __restrict__ x, const unsigned short* __restrict__ w,
                                                      unsigned short* __restrict__ out, int64_t M, int C, int64_t nunits) {
  const int lane = threadIdx.x & 63;
  const int64_t unit = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (unit >= nunits) return;
  const int G = C >> 5;
  const int g = (int)(unit % G);
  const int64_t m0 = (unit / G) * 32;
  const int hi = lane >> 5, l31 = lane & 31;
  int64_t m = m0 + l31;
  const bool live = m < M;
  if (!live) m = M - 1;
  f32x16_t acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) {
    const bf16x8_t af = *reinterpret_cast<const bf16x8_t*>(x + m * C + g * 32 + ks * 16 + hi * 8);
    const bf16x8_t wf = *reinterpret_cast<const bf16x8_t*>(w + (int64_t)(g * 32 + l31) * 32 + ks * 16 + hi * 8);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf, af, acc, 0, 0, 0);
  }
  if (!live) return;
#pragma unroll
  for (int qd = 0; qd < 4; ++qd) {
    uint2 o;
    o.x = pack_bf16x2(acc[qd * 4 + 0], acc[qd * 4 + 1]);
    o.y = pack_bf16x2(acc[qd * 4 + 2], acc[qd * 4 + 3]);
    *reinterpret_cast<uint2*>(out + m * C + g * 32 + qd * 8 + hi * 4) = o;
  }
}

// ---------------------------------------------------------------------------------------------------------------------------
// ReLU linear attention.  Pass 1: partial KV[d][j] = sum_n v[n][d] relu(k[n][j]) (d < 32), KV[32][j] = sum_n relu(k[n][j]) over a
// run of tokens, to ws[(bg * nsplit + s) * 1056 ...].  Pass 2: sums the partials (fixed order), out = KV relu(q) / (row 32 + eps).
constexpr int LA_KV = 33 * 32;

__global__ void __launch_bounds__(256) lin_attn_kv_kernel(const unsigned short* __restrict__ qkv, float* __restrict__ ws,
                                                          int N, int G, int per) {
  __shared__ __attribute__((aligned(16))) float sk[64][32];
  __shared__ __attribute__((aligned(16))) float sv[64][32];
  const int tid = threadIdx.x;
  const int s = blockIdx.x, nsplit = gridDim.x;
  const int bg = blockIdx.y;
  const int b = bg / G, g = bg - b * G;
  const int64_t rs = (int64_t)G * 96;
  const unsigned short* base = qkv + (int64_t)b * N * rs + g * 96 + 32;
  const int n_begin = s * per;
  const int n_end = n_begin + per < N ? n_begin + per : N;
  const int d = tid >> 3, jg = tid & 7;
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  float ksum = 0.f;
  for (int n0 = n_begin; n0 < n_end; n0 += 64) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int idx = tid + i * 256;
      const int tok = idx >> 3, c = idx & 7;
      float f[8];
      if (n0 + tok < n_end) {
        unpack8(*reinterpret_cast<const uint4*>(base + (int64_t)(n0 + tok) * rs + c * 8), f);
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) f[j] = 0.f;
      }
      if (c < 4) {
#pragma unroll
        for (int j = 0; j < 8; ++j) sk[tok][c * 8 + j] = fmaxf(f[j], 0.f);
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) sv[tok][(c - 4) * 8 + j] = f[j];
      }
    }
    __syncthreads();
#pragma unroll 8
    for (int n = 0; n < 64; ++n) {
      const float vv = sv[n][d];
      const float4 kk = *reinterpret_cast<const float4*>(&sk[n][jg * 4]);
      acc[0] = __builtin_fmaf(vv, kk.x, acc[0]);
      acc[1] = __builtin_fmaf(vv, kk.y, acc[1]);
      acc[2] = __builtin_fmaf(vv, kk.z, acc[2]);
      acc[3] = __builtin_fmaf(vv, kk.w, acc[3]);
    }
    if (tid < 32) {
      for (int n = 0; n < 64; ++n) ksum += sk[n][tid];
    }
    __syncthreads();
  }
  float* o = ws + ((int64_t)bg * nsplit + s) * LA_KV;
#pragma unroll
  for (int j = 0; j < 4; ++j) o[d * 32 + jg * 4 + j] = acc[j];
  if (tid < 32) o[32 * 32 + tid] = ksum;
}

__global__ void __launch_bounds__(256) lin_attn_out_kernel(const unsigned short* __restrict__ qkv, const float* __restrict__ ws,
                                                           unsigned short* __restrict__ out, int64_t out_row_stride,
                                                           int N, int G, int nsplit, float eps) {
  __shared__ __attribute__((aligned(16))) float skv[33][32];
  const int tid = threadIdx.x;
  const int bg = blockIdx.y;
  const int b = bg / G, g = bg - b * G;
  const float* part = ws + (int64_t)bg * nsplit * LA_KV;
  for (int e = tid; e < LA_KV; e += 256) {
    float t = 0.f;
    for (int s = 0; s < nsplit; ++s) t += part[(int64_t)s * LA_KV + e];
    skv[e >> 5][e & 31] = t;
  }
  __syncthreads();
  const int n = blockIdx.x * 256 + tid;
  if (n >= N) return;
  const int64_t row = (int64_t)b * N + n;
  const unsigned short* qp = qkv + row * ((int64_t)G * 96) + g * 96;
  float q[32];
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    unpack8(*reinterpret_cast<const uint4*>(qp + c * 8), q + c * 8);
#pragma unroll
    for (int j = 0; j < 8; ++j) q[c * 8 + j] = fmaxf(q[c * 8 + j], 0.f);
  }
  float den = 0.f;
#pragma unroll
  for (int j = 0; j < 32; ++j) den = __builtin_fmaf(skv[32][j], q[j], den);
  const float inv = 1.0f / (den + eps);
  unsigned short* op = out + row * out_row_stride + g * 32;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    float o[8];
#pragma unroll
    for (int dd = 0; dd < 8; ++dd) {
      float num = 0.f;
#pragma unroll
      for (int j = 0; j < 32; ++j) num = __builtin_fmaf(skv[c * 8 + dd][j], q[j], num);
      o[dd] = num * inv;
    }
    *reinterpret_cast<uint4*>(op + c * 8) = pack8(o);
  }
}

// ---------------------------------------------------------------------------------------------------------------------------
// RMSNorm over channels: one wave per token.  out = act(x * rsqrt(mean(x^2) + eps) * w + b) + res
__global__ void __launch_bounds__(256) rmsnorm_affine_kernel(const unsigned short* __restrict__ x, const float* __restrict__ w,
                                                             const float* __restrict__ bias, const unsigned short* __restrict__ res,
                                                             unsigned short* __restrict__ out, int64_t M, int C, float eps, int relu) {
  const int lane = threadIdx.x & 63;
  const int64_t m = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (m >= M) return;
  const unsigned short* xr = x + m * C;
  const int chunks = C >> 3;
  float ss = 0.f;
  for (int c = lane; c < chunks; c += 64) {
    float f[8];
    unpack8(*reinterpret_cast<const uint4*>(xr + c * 8), f);
#pragma unroll
    for (int j = 0; j < 8; ++j) ss = __builtin_fmaf(f[j], f[j], ss);
  }
  ss = wave_sum(ss);
  const float rstd = 1.0f / sqrtf(ss / (float)C + eps);
  for (int c = lane; c < chunks; c += 64) {
    float f[8];
    unpack8(*reinterpret_cast<const uint4*>(xr + c * 8), f);
    const float4 w0 = *reinterpret_cast<const float4*>(w + c * 8), w1 = *reinterpret_cast<const float4*>(w + c * 8 + 4);
    const float4 b0 = *reinterpret_cast<const float4*>(bias + c * 8), b1 = *reinterpret_cast<const float4*>(bias + c * 8 + 4);
    const float wv[8] = {w0.x, w0.y, w0.z, w0.w, w1.x, w1.y, w1.z, w1.w};
    const float bv[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      f[j] = __builtin_fmaf(f[j] * rstd, wv[j], bv[j]);
      if (relu) f[j] = fmaxf(f[j], 0.f);
    }
    if (res) {
      float r[8];
      unpack8(*reinterpret_cast<const uint4*>(res + m * C + c * 8), r);
#pragma unroll
      for (int j = 0; j < 8; ++j) f[j] += r[j];
    }
    *reinterpret_cast<uint4*>(out + m * C + c * 8) = pack8(f);
  }
}

inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }
constexpr int64_t MAX_BLOCKS = (int64_t)1 << 31;

}  // namespace

extern "C" int osk_conv3d_zp_ndhwc_bf16(const void* x, int B, int T, int H, int W, int Cin, const void* w, int64_t w_row_stride,
                                        const float* bias, int Cout, int ksize, int up_t, int up_hw, int act, const void* res,
                                        void* out, void* stream) {
  if (!x || !w || !out || B <= 0 || T <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0) return OSK_EINVAL;
  if (ksize != 1 && ksize != 3) return OSK_EINVAL;
  if ((up_t != 0 && up_t != 1) || (up_hw != 0 && up_hw != 1) || (act != 0 && act != 1)) return OSK_EINVAL;
  if ((Cin & 7) || (Cin & (Cin - 1))) return OSK_EUNSUPPORTED;  // Cin = 8 * 2^j
  if (!al16(x) || !al16(w) || !al16(bias) || ((uintptr_t)out & 7) || ((uintptr_t)res & 7)) return OSK_EINVAL;
  Conv3dParams p;
  p.x = (const unsigned short*)x; p.w = (const unsigned short*)w; p.bias = bias;
  p.res = (const unsigned short*)res; p.out = (unsigned short*)out;
  p.T = T; p.H = H; p.W = W; p.Cout = Cout;
  p.ut = up_t; p.uh = up_hw; p.act = act; p.ks = ksize;
  const int64_t Tu = (int64_t)T << up_t, Hu = (int64_t)H << up_hw, Wu = (int64_t)W << up_hw;
  const int64_t M = (int64_t)B * Tu * Hu * Wu;
  if (M >= (int64_t)1 << 31 || (int64_t)B * T * H * W * Cin >= (int64_t)1 << 34) return OSK_EUNSUPPORTED;
  p.Tu = (int)Tu; p.Hu = (int)Hu; p.Wu = (int)Wu;
  p.M = (int)M;
  p.brick = (Hu % 8 == 0 && Wu % 16 == 0) ? 1 : 0;
  p.ntaps = ksize * ksize * ksize;
  if (conv_k_layout(Cin, p.ntaps, w_row_stride, &p.lg_cpt, &p.nk) != OSK_OK) return OSK_EINVAL;
  p.wrs = w_row_stride;
  const int64_t nblk = ((M + BM - 1) / BM) * ((Cout + BN - 1) / BN);
  if (nblk >= MAX_BLOCKS) return OSK_EUNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  dim3 grid((unsigned)nblk), block(256);
  if (Cin % 64 == 0) hipLaunchKernelGGL((conv3d_zp_kernel<Conv3dASrc<true>>), grid, block, SMEM_BYTES, s, p);
  else hipLaunchKernelGGL((conv3d_zp_kernel<Conv3dASrc<false>>), grid, block, SMEM_BYTES, s, p);
  return (int)hipGetLastError();
}

extern "C" int osk_conv3d_zp_strided_ndhwc_bf16(const void* x, int B, int T, int H, int W, int Cin, const void* w,
                                                int64_t w_row_stride, const float* bias, int Cout, int stride_t, int stride_hw,
                                                const void* res, void* out, void* stream) {
  if (!x || !w || !out || B <= 0 || T <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0) return OSK_EINVAL;
  if ((stride_t != 1 && stride_t != 2) || stride_hw != 2) return OSK_EINVAL;
  if ((Cin & 7) || (Cin & (Cin - 1))) return OSK_EUNSUPPORTED;  // Cin = 8 * 2^j
  if (!al16(x) || !al16(w) || !al16(bias) || ((uintptr_t)out & 7) || ((uintptr_t)res & 7)) return OSK_EINVAL;
  Conv3dParams p;
  p.x = (const unsigned short*)x; p.w = (const unsigned short*)w; p.bias = bias;
  p.res = (const unsigned short*)res; p.out = (unsigned short*)out;
  p.T = T; p.H = H; p.W = W; p.Cout = Cout;
  p.ut = 0; p.uh = 0; p.act = 0; p.ks = 3;
  p.st = stride_t; p.sh = stride_hw;
  const int64_t To = (T - 1) / stride_t + 1, Ho = (H - 1) / stride_hw + 1, Wo = (W - 1) / stride_hw + 1;
  const int64_t M = (int64_t)B * To * Ho * Wo;
  if ((int64_t)B * T * H * W >= (int64_t)1 << 31 || (int64_t)B * T * H * W * Cin >= (int64_t)1 << 34) return OSK_EUNSUPPORTED;
  p.Tu = (int)To; p.Hu = (int)Ho; p.Wu = (int)Wo;
  p.M = (int)M;
  p.brick = (Ho % 8 == 0 && Wo % 16 == 0) ? 1 : 0;
  p.ntaps = 27;
  if (conv_k_layout(Cin, p.ntaps, w_row_stride, &p.lg_cpt, &p.nk) != OSK_OK) return OSK_EINVAL;
  p.wrs = w_row_stride;
  const int64_t nblk = ((M + BM - 1) / BM) * ((Cout + BN - 1) / BN);
  if (nblk >= MAX_BLOCKS) return OSK_EUNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  dim3 grid((unsigned)nblk), block(256);
  if (Cin % 64 == 0) hipLaunchKernelGGL((conv3d_zp_kernel<Conv3dStridedASrc<true>>), grid, block, SMEM_BYTES, s, p);
  else hipLaunchKernelGGL((conv3d_zp_kernel<Conv3dStridedASrc<false>>), grid, block, SMEM_BYTES, s, p);
  return (int)hipGetLastError();
}

extern "C" int osk_unshuffle_avg_ndhwc_bf16(const void* x, int B, int T, int H, int W, int Cin, void* out, int Cout, int ft, int fhw,
                                            void* stream) {
  if (!x || !out || B <= 0 || T <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0) return OSK_EINVAL;
  if ((ft != 1 && ft != 2) || (fhw != 1 && fhw != 2)) return OSK_EINVAL;
  if (T % ft || H % fhw || W % fhw || !al16(out)) return OSK_EINVAL;
  if (Cout & 7) return OSK_EUNSUPPORTED;
  const int64_t per = (int64_t)ft * fhw * fhw;
  if ((Cin * per) % Cout) return OSK_EINVAL;
  const int64_t gs = Cin * per / Cout;
  const int64_t total = (int64_t)B * (T / ft) * (H / fhw) * (W / fhw) * (Cout >> 3);
  const int64_t nblk = (total + 255) / 256;
  if (nblk >= MAX_BLOCKS || Cin * per >= (int64_t)1 << 31) return OSK_EUNSUPPORTED;
  hipLaunchKernelGGL(unshuffle_avg_kernel, dim3((unsigned)nblk), dim3(256), 0, (hipStream_t)stream, (const unsigned short*)x,
                     (unsigned short*)out, T / ft, H / fhw, W / fhw, Cin, Cout, ft, fhw, (int)gs, 1.0f / (float)gs, total);
  return (int)hipGetLastError();
}

extern "C" int osk_dup_shuffle_ndhwc_bf16(const void* x, int B, int T, int H, int W, int Cin, void* out, int Cout, int ft, int fhw,
                                          void* stream) {
  if (!x || !out || B <= 0 || T <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0) return OSK_EINVAL;
  if ((ft != 1 && ft != 2) || (fhw != 1 && fhw != 2)) return OSK_EINVAL;
  if (!al16(out)) return OSK_EINVAL;
  if (Cout & 7) return OSK_EUNSUPPORTED;
  const int64_t per = (int64_t)ft * fhw * fhw;
  if ((Cout * per) % Cin) return OSK_EINVAL;
  const int rep = (int)(Cout * per / Cin);
  const int64_t total = (int64_t)B * T * ft * H * fhw * W * fhw * (Cout >> 3);
  const int64_t nblk = (total + 255) / 256;
  if (nblk >= MAX_BLOCKS || Cout * per >= (int64_t)1 << 31) return OSK_EUNSUPPORTED;
  hipLaunchKernelGGL(dup_shuffle_kernel, dim3((unsigned)nblk), dim3(256), 0, (hipStream_t)stream, (const unsigned short*)x,
                     (unsigned short*)out, T, H, W, Cin, Cout, ft, fhw, rep, total);
  return (int)hipGetLastError();
}

extern "C" int osk_dwconv3d_ndhwc_bf16(const void* x, int B, int T, int H, int W, int C, const void* w, const float* bias, int ksize,
                                       int glu, void* out, void* stream) {
  if (!x || !w || !out || B <= 0 || T <= 0 || H <= 0 || W <= 0 || C <= 0) return OSK_EINVAL;
  if ((glu != 0 && glu != 1) || !al16(x) || !al16(w) || !al16(out)) return OSK_EINVAL;
  if (ksize != 3 && ksize != 5) return OSK_EUNSUPPORTED;
  if (C % (glu ? 16 : 8)) return OSK_EUNSUPPORTED;
  const int Co = glu ? C / 2 : C;
  const int64_t total = (int64_t)B * T * H * W * (Co >> 3);
  const int64_t nblk = (total + 255) / 256;
  if (nblk >= MAX_BLOCKS) return OSK_EUNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  dim3 grid((unsigned)nblk), block(256);
  const unsigned short* xp = (const unsigned short*)x;
  const unsigned short* wp = (const unsigned short*)w;
  unsigned short* op = (unsigned short*)out;
  if (ksize == 3 && glu) hipLaunchKernelGGL((dwconv3d_kernel<3, true>), grid, block, 0, s, xp, wp, bias, op, T, H, W, C, total);
  else if (ksize == 3) hipLaunchKernelGGL((dwconv3d_kernel<3, false>), grid, block, 0, s, xp, wp, bias, op, T, H, W, C, total);
  else if (glu) hipLaunchKernelGGL((dwconv3d_kernel<5, true>), grid, block, 0, s, xp, wp, bias, op, T, H, W, C, total);
  else hipLaunchKernelGGL((dwconv3d_kernel<5, false>), grid, block, 0, s, xp, wp, bias, op, T, H, W, C, total);
  return (int)hipGetLastError();
}

extern "C" int osk_gconv32_bf16(const void* x, int64_t M, int C, const void* w, void* out, void* stream) {
  if (!x || !w || !out || M <= 0 || C <= 0) return OSK_EINVAL;
  if (!al16(x) || !al16(w) || !al16(out)) return OSK_EINVAL;
  if (C & 31) return OSK_EUNSUPPORTED;
  const int64_t nunits = ((M + 31) / 32) * (C >> 5);
  const int64_t nblk = (nunits + 3) / 4;
  if (nblk >= MAX_BLOCKS) return OSK_EUNSUPPORTED;
  hipLaunchKernelGGL(gconv32_kernel, dim3((unsigned)nblk), dim3(256), 0, (hipStream_t)stream, (const unsigned short*)x,
                     (const unsigned short*)w, (unsigned short*)out, M, C, nunits);
  return (int)hipGetLastError();
}

extern "C" int osk_relu_linear_attn_bf16(const void* qkv, int B, int N, int G, void* out, int64_t out_row_stride, float* workspace,
                                         int64_t workspace_bytes, int nsplit, float eps, void* stream) {
  if (!qkv || !out || !workspace || B <= 0 || N <= 0 || G <= 0 || nsplit <= 0) return OSK_EINVAL;
  if (!al16(qkv) || !al16(out) || !al16(workspace) || (out_row_stride & 7) || out_row_stride < (int64_t)G * 32) return OSK_EINVAL;
  if ((int64_t)B * G > 65535 || nsplit > 1024) return OSK_EUNSUPPORTED;
  if (workspace_bytes < (int64_t)B * G * nsplit * LA_KV * 4) return OSK_EINVAL;
  int per = (N + nsplit - 1) / nsplit;
  per = (per + 63) / 64 * 64;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(lin_attn_kv_kernel, dim3(nsplit, B * G), dim3(256), 0, s, (const unsigned short*)qkv, workspace, N, G, per);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(lin_attn_out_kernel, dim3((N + 255) / 256, B * G), dim3(256), 0, s, (const unsigned short*)qkv, workspace,
                     (unsigned short*)out, out_row_stride, N, G, nsplit, eps);
  return (int)hipGetLastError();
}

extern "C" int osk_rmsnorm_affine_bf16(const void* x, int64_t M, int C, const float* weight, const float* bias, float eps,
                                       const void* res, int relu, void* out, void* stream) {
  if (!x || !weight || !bias || !out || M <= 0 || C <= 0) return OSK_EINVAL;
  if (!al16(x) || !al16(weight) || !al16(bias) || !al16(res) || !al16(out) || (relu != 0 && relu != 1)) return OSK_EINVAL;
  if (C & 7) return OSK_EUNSUPPORTED;
  const int64_t nblk = (M + 3) / 4;
  if (nblk >= MAX_BLOCKS) return OSK_EUNSUPPORTED;
  hipLaunchKernelGGL(rmsnorm_affine_kernel, dim3((unsigned)nblk), dim3(256), 0, (hipStream_t)stream, (const unsigned short*)x, weight,
                     bias, (const unsigned short*)res, (unsigned short*)out, M, C, eps, relu);
  return (int)hipGetLastError();
}
