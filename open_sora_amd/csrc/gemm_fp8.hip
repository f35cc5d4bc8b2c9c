// FP8 (OCP e4m3fn) GEMM path for gfx950: dynamic per-row quantisation of bf16 activations and the C-ABI entry of the
// fp8 instantiation of the large-tile hand-scheduled GEMM (gemm256.hip, K loop gemm256_fp8_body_n*.inc).
//
// Scheme (BASELINE configs[4] asks for "fp8 MFMA"; the reference itself is bf16, so this is an opt-in mode whose error
// is reported against the bf16 path, SURVEY.md 8(d) "Parity tolerance"):
//   activations: one f32 scale per token row,   sa[m] = absmax(A[m, :]) / 448,  A8 = e4m3(A / sa)      (this file)
//   weights:     one f32 scale per output row,  sw[n] = absmax(W[n, :]) / 448,  W8 = e4m3(W / sw)      (same kernel,
//                once at load time)
//   C[m, n] = epilogue(sa[m] * sw[n] * sum_k A8[m, k] W8[n, k] + bias[n])        f32 accumulate on the MFMA
#include "gemm_params.h"
#include "../../include/osk.h"

namespace {

// one wave per row; two passes over the row (the second one hits L2): absmax, then scale + convert + store.
// Algorithmic bytes: 3 * M * K (read bf16, write e4m3) + 4 M.
__global__ void __launch_bounds__(256) quantize_rows_fp8_kernel(const unsigned short* __restrict__ x, int64_t xbs,
                                                                int64_t xrs, int rpb, unsigned char* __restrict__ out,
                                                                float* __restrict__ scales, int M, int K) {
  const int lane = threadIdx.x & 63;
  const int m = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (m >= M) return;
  const int b = m / rpb, l = m - b * rpb;
  const unsigned short* row = x + b * xbs + (int64_t)l * xrs;
  const int nch = K >> 3;
  float amax = 0.f;
  for (int c = lane; c < nch; c += 64) {
    const uint4 u = *reinterpret_cast<const uint4*>(row + c * 8);
    float f[8];
    unpack8(u, f);
#pragma unroll
    for (int j = 0; j < 8; ++j) amax = fmaxf(amax, fabsf(f[j]));
  }
  amax = wave_max(amax);
  const float inv = amax > 0.f ? 448.0f / amax : 0.f;
  if (lane == 0) scales[m] = amax > 0.f ? amax / 448.0f : 1.0f;
  unsigned char* orow = out + (int64_t)m * K;
  for (int c = lane; c < nch; c += 64) {
    const uint4 u = *reinterpret_cast<const uint4*>(row + c * 8);
    float f[8];
    unpack8(u, f);
#pragma unroll
    for (int j = 0; j < 8; ++j) f[j] = fminf(fmaxf(f[j] * inv, -448.0f), 448.0f);
    int w0 = 0, w1 = 0;
    w0 = __builtin_amdgcn_cvt_pk_fp8_f32(f[0], f[1], w0, false);
    w0 = __builtin_amdgcn_cvt_pk_fp8_f32(f[2], f[3], w0, true);
    w1 = __builtin_amdgcn_cvt_pk_fp8_f32(f[4], f[5], w1, false);
    w1 = __builtin_amdgcn_cvt_pk_fp8_f32(f[6], f[7], w1, true);
    *reinterpret_cast<uint2*>(orow + c * 8) = make_uint2((unsigned)w0, (unsigned)w1);
  }
}

}  // namespace

extern "C" int osk_quantize_rows_fp8(const void* x, int64_t x_batch_stride, int64_t x_row_stride, int rows_per_batch,
                                     void* out8, float* scales, int M, int K, void* stream) {
  if (!x || !out8 || !scales || M <= 0 || K <= 0 || rows_per_batch <= 0) return OSK_EINVAL;
  if ((K & 7) || (x_batch_stride & 7) || (x_row_stride & 7) || ((uintptr_t)x & 15) || ((uintptr_t)out8 & 7))
    return OSK_EINVAL;
  dim3 grid((M + 3) / 4), block(256);
  hipLaunchKernelGGL(quantize_rows_fp8_kernel, grid, block, 0, (hipStream_t)stream, (const unsigned short*)x,
                     x_batch_stride, x_row_stride, rows_per_batch, (unsigned char*)out8, scales, M, K);
  return (int)hipGetLastError();
}

extern "C" int osk_gemm_fp8(const void* A8, int64_t a_batch_stride, int64_t a_row_stride, int a_rows_per_batch,
                            const float* a_scale, const void* W8, int64_t w_row_stride, const float* w_scale,
                            const float* bias, void* C, int64_t c_batch_stride, int64_t c_row_stride,
                            int c_rows_per_batch, const void* res, const float* gate, int64_t gate_batch_stride,
                            int M, int N, int K, int gelu_from, int out_f32, void* stream) {
  using osk_gemm::GemmParams;
  if (!A8 || !W8 || !C || !a_scale || !w_scale || M <= 0 || N <= 0 || K <= 0) return OSK_EINVAL;
  if (a_rows_per_batch <= 0 || c_rows_per_batch <= 0) return OSK_EINVAL;
  if ((a_batch_stride & 15) || (a_row_stride & 15) || (w_row_stride & 15)) return OSK_EINVAL;
  if ((c_batch_stride & 3) || (c_row_stride & 3)) return OSK_EINVAL;
  if (((uintptr_t)A8 & 15) || ((uintptr_t)W8 & 15) || ((uintptr_t)C & 7) || ((uintptr_t)bias & 15) ||
      ((uintptr_t)w_scale & 15))
    return OSK_EINVAL;
  if (gate && (!res || ((uintptr_t)gate & 15) || (gate_batch_stride & 3) || ((uintptr_t)res & 7))) return OSK_EINVAL;
  if (out_f32 && ((uintptr_t)C & 15)) return OSK_EINVAL;   // the f32 epilogue stores float4
  GemmParams p;
  p.A = (const unsigned short*)A8; p.abs_ = a_batch_stride; p.ars = a_row_stride; p.arpb = a_rows_per_batch;
  p.W = (const unsigned short*)W8; p.wrs = w_row_stride; p.bias = bias;
  p.C = C; p.cbs = c_batch_stride; p.crs = c_row_stride; p.crpb = c_rows_per_batch;
  p.res = (const unsigned short*)res; p.gate = gate; p.gbs = gate_batch_stride;
  p.M = M; p.N = N; p.K = K; p.gelu_from = gelu_from;
  p.sa = a_scale; p.sw = w_scale;
  p.group = (N + 255) / 256 <= 6 ? 4 : 8;
  // only the large-tile kernel has an fp8 instantiation: small / odd shapes stay on osk_gemm_bf16 (the host decides)
  if (!osk_gemm::gemm256_fp8_supported(p)) return OSK_EUNSUPPORTED;
  auto rounds = [](int64_t tiles, int64_t slots) { return (double)((tiles + slots - 1) / slots); };
  const int64_t m256 = (M + 255) / 256;
  const double c256 = rounds(m256 * ((N + 255) / 256), 256) * 4.0;
  const double c128 = rounds(m256 * ((N + 127) / 128), 256) * 2.0 / 0.78;
  const int bn = (N >= 256 && c256 <= c128) ? 256 : 128;
  return osk_gemm::launch_gemm256_fp8(p, bn, out_f32, (hipStream_t)stream);
}
