// LayerNorm over channels with affine weight and bias (nn.LayerNorm: CLIP's text tower, conditioner.py:17-20, 48-53), gfx950.
//   out[m, :] = bf16((x[m, :] - mean) * rsqrt(var + eps) * w + b),   var = mean((x - mean)^2)  (biased)
//
// A row kernel, HBM / launch bound: one wave per row, four rows per workgroup.  The row is read ONCE, 16 bytes per lane and chunk,
// and stays in registers (NCH chunks of 8 channels per lane: C <= 512 NCH) through both statistics passes: the mean first, then the
// variance of the CENTRED values.  E[x^2] - mean^2 is not used: on a constant row of 300 it is 90000 - 90000 with an f32 rounding
// error of either sign, and a negative variance below -eps is a NaN.  Centred, a constant row has variance exactly 0 and comes out
// as bf16(bias).
#include "../../include/osk.h"
#include "osk_common.h"

namespace {

template <int NCH>
__global__ void __launch_bounds__(256) layernorm_affine_kernel(const unsigned short* __restrict__ x, int64_t xrs,
                                                               unsigned short* __restrict__ out, int64_t ors,
                                                               const float* __restrict__ w, const float* __restrict__ bias, int64_t M,
                                                               int C, float eps) {
  const int lane = threadIdx.x & 63;
  const int64_t m = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (m >= M) return;
  const unsigned short* xr = x + m * xrs;
  const int chunks = C >> 3;
  float f[NCH][8];
  float sum = 0.f;
#pragma unroll
  for (int i = 0; i < NCH; ++i) {
    const int c = lane + 64 * i;
    if (c < chunks) {
      unpack8(*reinterpret_cast<const uint4*>(xr + c * 8), f[i]);
#pragma unroll
      for (int j = 0; j < 8; ++j) sum += f[i][j];
    }
  }
  const float mean = wave_sum(sum) / (float)C;   // a true division: the mean of a constant row is that constant, exactly
  float ss = 0.f;
#pragma unroll
  for (int i = 0; i < NCH; ++i) {
    if (lane + 64 * i < chunks) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        f[i][j] -= mean;
        ss = __builtin_fmaf(f[i][j], f[i][j], ss);
      }
    }
  }
  const float rstd = 1.0f / sqrtf(wave_sum(ss) / (float)C + eps);
  unsigned short* orow = out + m * ors;
#pragma unroll
  for (int i = 0; i < NCH; ++i) {
    const int c = lane + 64 * i;
    if (c < chunks) {
      const float4 w0 = *reinterpret_cast<const float4*>(w + c * 8), w1 = *reinterpret_cast<const float4*>(w + c * 8 + 4);
      const float4 b0 = *reinterpret_cast<const float4*>(bias + c * 8), b1 = *reinterpret_cast<const float4*>(bias + c * 8 + 4);
      const float wv[8] = {w0.x, w0.y, w0.z, w0.w, w1.x, w1.y, w1.z, w1.w};
      const float bv[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
      float o[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) o[j] = __builtin_fmaf(f[i][j] * rstd, wv[j], bv[j]);
      *reinterpret_cast<uint4*>(orow + c * 8) = pack8(o);
    }
  }
}

constexpr int LN_MAX_C = 512 * 8;   // 8 chunks per lane: 64 f32 registers of row

}  // namespace

extern "C" int osk_layernorm_affine_bf16(const void* x, int64_t x_row_stride, void* out, int64_t out_row_stride, const float* weight,
                                         const float* bias, int64_t M, int C, float eps, void* stream) {
  if (!x || !out || !weight || !bias || M <= 0 || C <= 0) return OSK_EINVAL;
  if ((C & 7) || C > LN_MAX_C) return OSK_EUNSUPPORTED;
  if (x_row_stride < C || out_row_stride < C || (x_row_stride & 7) || (out_row_stride & 7)) return OSK_EINVAL;
  if (((uintptr_t)x & 15) || ((uintptr_t)out & 15) || ((uintptr_t)weight & 15) || ((uintptr_t)bias & 15)) return OSK_EINVAL;
  const int64_t nblk = (M + 3) / 4;
  if (nblk > 0x7FFFFFFF) return OSK_EUNSUPPORTED;
  const int nch = (C / 8 + 63) / 64;
  const dim3 grid((unsigned)nblk), block(256);
  hipStream_t st = (hipStream_t)stream;
  const unsigned short* xp = (const unsigned short*)x;
  unsigned short* op = (unsigned short*)out;
  if (nch <= 1) hipLaunchKernelGGL(layernorm_affine_kernel<1>, grid, block, 0, st, xp, x_row_stride, op, out_row_stride, weight, bias, M, C, eps);
  else if (nch <= 2) hipLaunchKernelGGL(layernorm_affine_kernel<2>, grid, block, 0, st, xp, x_row_stride, op, out_row_stride, weight, bias, M, C, eps);
  else if (nch <= 4) hipLaunchKernelGGL(layernorm_affine_kernel<4>, grid, block, 0, st, xp, x_row_stride, op, out_row_stride, weight, bias, M, C, eps);
  else hipLaunchKernelGGL(layernorm_affine_kernel<8>, grid, block, 0, st, xp, x_row_stride, op, out_row_stride, weight, bias, M, C, eps);
  return (int)hipGetLastError();
}
