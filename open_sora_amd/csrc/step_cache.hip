// Step cache of the sampler (I2VDenoiser.denoise(step_cache=...)): the relative-L1 distance between two consecutive steps' block-0
// inputs, and the residual of the block stack that a skipped step re-applies.  All HBM-bound, 16 B per lane, f32 math.
#include "osk_common.h"
#include "../../include/osk.h"

// =============================================================================================
// Step delta: sums[0] = sum |cur - prev|, sums[1] = sum |prev| over bf16 [B, L, C]; prev := cur in the same pass.
// Two stages, no atomics, so two calls on equal inputs give equal bits:
//   stage 1  G = step_delta_blocks(chunks) workgroups of 256 lanes walk the 8-element chunks grid-stride; a lane adds its chunks'
//            16 terms one after the other, the wave adds its lanes by a 6-step butterfly, lane 0 adds the 4 waves in order and
//            writes the workgroup's pair to partials[2 g], partials[2 g + 1];
//   stage 2  one workgroup: lane t adds partials t, t + 256, ... in order, then the same wave / workgroup finish.
// G depends on the shape only.  Longest chain of f32 roundings from a term to a sum (the tolerance of tests/test_gpu_step_cache.py):
//   1 (the difference) + 8 ceil(chunks / (256 G)) + 6 + 3  +  ceil(G / 256) + 6 + 3.
// Bytes: 6 per element (cur read, prev read, prev written) + 8 G written and read.
// =============================================================================================
#define STEP_DELTA_MAX_BLOCKS 2048

static inline int64_t step_delta_blocks(int64_t chunks) {
  const int64_t g = (chunks + 255) / 256;
  return g < 1 ? 1 : (g > STEP_DELTA_MAX_BLOCKS ? STEP_DELTA_MAX_BLOCKS : g);
}

// the workgroup's sum of (a, b) in lane 0 of wave 0: butterfly per wave, then the four waves in order
OSK_DEV void block_sum2(float& a, float& b, float (*sh)[2]) {
  a = wave_sum(a);
  b = wave_sum(b);
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    sh[w][0] = a;
    sh[w][1] = b;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    a = ((sh[0][0] + sh[1][0]) + sh[2][0]) + sh[3][0];
    b = ((sh[0][1] + sh[1][1]) + sh[2][1]) + sh[3][1];
  }
}

__global__ void __launch_bounds__(256) step_delta_kernel(const unsigned short* __restrict__ cur, int64_t cbs, int64_t crs,
                                                         unsigned short* __restrict__ prev, float* __restrict__ partials,
                                                         unsigned L, unsigned C8, unsigned chunks) {
  __shared__ float sh[4][2];
  const unsigned per_b = L * C8;              // chunks of one batch item (B L C / 8 < 2^31: checked by the entry point)
  const bool rows_dense = crs == (int64_t)C8 * 8;
  float num = 0.f, den = 0.f;
  for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < chunks; i += gridDim.x * 256u) {
    const unsigned b = i / per_b, r = i - b * per_b;
    int64_t off;
    if (rows_dense) {
      off = b * cbs + (int64_t)r * 8;
    } else {
      const unsigned l = r / C8, c = r - l * C8;
      off = b * cbs + l * crs + (int64_t)c * 8;
    }
    const uint4 uc = *reinterpret_cast<const uint4*>(cur + off);
    uint4* pp = reinterpret_cast<uint4*>(prev + (int64_t)i * 8);
    const uint4 up = *pp;
    float fc[8], fp[8];
    unpack8(uc, fc);
    unpack8(up, fp);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      num += fabsf(fc[j] - fp[j]);
      den += fabsf(fp[j]);
    }
    *pp = uc;
  }
  block_sum2(num, den, sh);
  if (threadIdx.x == 0) {
    partials[2 * blockIdx.x] = num;
    partials[2 * blockIdx.x + 1] = den;
  }
}

__global__ void __launch_bounds__(256) step_delta_finish_kernel(const float* __restrict__ partials, int G, float* __restrict__ sums) {
  __shared__ float sh[4][2];
  float num = 0.f, den = 0.f;
  for (int g = threadIdx.x; g < G; g += 256) {
    num += partials[2 * g];
    den += partials[2 * g + 1];
  }
  block_sum2(num, den, sh);
  if (threadIdx.x == 0) {
    sums[0] = num;
    sums[1] = den;
  }
}

extern "C" int64_t osk_step_delta_workspace_bytes(int B, int L, int C) {
  if (B <= 0 || L <= 0 || C <= 0 || (C & 7)) return 0;
  return step_delta_blocks((int64_t)B * L * (C / 8)) * 2 * (int64_t)sizeof(float);
}

extern "C" int osk_step_delta_bf16(const void* cur, int64_t cur_batch_stride, int64_t cur_row_stride, void* prev, float* sums, int B,
                                   int L, int C, void* workspace, int64_t workspace_bytes, void* stream) {
  if (!cur || !prev || !sums || !workspace || B <= 0 || L <= 0 || C <= 0 || (C & 7)) return OSK_EINVAL;
  if ((cur_batch_stride & 7) || (cur_row_stride & 7) || cur_row_stride < C || (B > 1 && cur_batch_stride < (int64_t)L * cur_row_stride))
    return OSK_EINVAL;
  if (((uintptr_t)cur & 15) || ((uintptr_t)prev & 15) || ((uintptr_t)sums & 3) || ((uintptr_t)workspace & 3)) return OSK_EINVAL;
  const int64_t chunks = (int64_t)B * L * (C / 8);
  if (chunks >= (1ll << 31)) return OSK_EINVAL;
  const int64_t G = step_delta_blocks(chunks);
  if (workspace_bytes < G * 2 * (int64_t)sizeof(float)) return OSK_EINVAL;
  hipLaunchKernelGGL(step_delta_kernel, dim3((unsigned)G), dim3(256), 0, (hipStream_t)stream, (const unsigned short*)cur,
                     cur_batch_stride, cur_row_stride, (unsigned short*)prev, (float*)workspace, (unsigned)L, (unsigned)(C / 8),
                     (unsigned)chunks);
  hipLaunchKernelGGL(step_delta_finish_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const float*)workspace, (int)G, sums);
  return (int)hipGetLastError();
}

// =============================================================================================
// Sums combine (the step cache under sequence parallelism): every rank's osk_step_delta_bf16 gives the pair of its own rows; the P
// pairs, gathered as f32 [P, 2], are added in rank order 0 .. P-1 by ONE lane with plain f32 adds: sums[0] = ((p[0][0] + p[1][0]) +
// ...) + p[P-1][0], sums[1] likewise.  Every rank holds the same gathered bits and runs the same P - 1 adds, so the sums -- and the
// decision the host takes from them -- are equal bit for bit on all ranks.  A NaN or an infinity in any pair reaches the sum.
// =============================================================================================
__global__ void __launch_bounds__(64) step_sums_combine_kernel(const float* __restrict__ pairs, int P, float* __restrict__ sums) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  float num = pairs[0], den = pairs[1];
  for (int r = 1; r < P; ++r) {
    num += pairs[2 * r];
    den += pairs[2 * r + 1];
  }
  sums[0] = num;
  sums[1] = den;
}

extern "C" int osk_step_sums_combine_f32(const float* pairs, int P, float* sums, void* stream) {
  if (!pairs || !sums || P < 1) return OSK_EINVAL;
  if (((uintptr_t)pairs & 3) || ((uintptr_t)sums & 3)) return OSK_EINVAL;
  hipLaunchKernelGGL(step_sums_combine_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, pairs, P, sums);
  return (int)hipGetLastError();
}

// =============================================================================================
// Residual store / apply: out = bf16(f32(a) - f32(b)) or bf16(f32(a) + f32(b)) over strided bf16 [B, L, C] views.  The f32 sum of
// two bf16 values is exact unless their exponents are 16 or more apart, and then the smaller one is far below half a bf16 step of
// the larger: the result is the exact sum rounded once.  out may be a or b themselves (same strides): a lane reads its 8
// elements before it writes them.  Bytes: 6 per element.
// =============================================================================================
template <bool ADD>
__global__ void __launch_bounds__(256) residual_kernel(const unsigned short* a, int64_t abs_, int64_t ars, const unsigned short* b,
                                                       int64_t bbs, int64_t brs, unsigned short* out, int64_t obs, int64_t ors,
                                                       unsigned L, unsigned C8, unsigned chunks) {
  const unsigned per_b = L * C8;
  for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < chunks; i += gridDim.x * 256u) {
    const unsigned bi = i / per_b, r = i - bi * per_b;
    const unsigned l = r / C8;
    const int64_t c = (int64_t)(r - l * C8) * 8;
    float fa[8], fb[8], o[8];
    unpack8(*reinterpret_cast<const uint4*>(a + bi * abs_ + l * ars + c), fa);
    unpack8(*reinterpret_cast<const uint4*>(b + bi * bbs + l * brs + c), fb);
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = ADD ? fa[j] + fb[j] : fa[j] - fb[j];
    *reinterpret_cast<uint4*>(out + bi * obs + l * ors + c) = pack8(o);
  }
}

static bool view_ok(const void* p, int64_t bs, int64_t rs, int B, int L, int C) {
  return p && !((uintptr_t)p & 15) && !(bs & 7) && !(rs & 7) && rs >= C && (B == 1 || bs >= (int64_t)L * rs);
}

template <bool ADD>
static int residual_launch(const void* a, int64_t a_bs, int64_t a_rs, const void* b, int64_t b_bs, int64_t b_rs, void* out, int64_t o_bs,
                           int64_t o_rs, int B, int L, int C, void* stream) {
  if (B <= 0 || L <= 0 || C <= 0 || (C & 7)) return OSK_EINVAL;
  if (!view_ok(a, a_bs, a_rs, B, L, C) || !view_ok(b, b_bs, b_rs, B, L, C) || !view_ok(out, o_bs, o_rs, B, L, C)) return OSK_EINVAL;
  const int64_t chunks = (int64_t)B * L * (C / 8);
  if (chunks >= (1ll << 31)) return OSK_EINVAL;
  int64_t nb = (chunks + 255) / 256;
  if (nb > 2048) nb = 2048;
  hipLaunchKernelGGL(residual_kernel<ADD>, dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, (const unsigned short*)a, a_bs, a_rs,
                     (const unsigned short*)b, b_bs, b_rs, (unsigned short*)out, o_bs, o_rs, (unsigned)L, (unsigned)(C / 8), (unsigned)chunks);
  return (int)hipGetLastError();
}

extern "C" int osk_residual_sub_bf16(const void* a, int64_t a_batch_stride, int64_t a_row_stride, const void* b, int64_t b_batch_stride,
                                     int64_t b_row_stride, void* out, int64_t out_batch_stride, int64_t out_row_stride, int B, int L, int C,
                                     void* stream) {
  return residual_launch<false>(a, a_batch_stride, a_row_stride, b, b_batch_stride, b_row_stride, out, out_batch_stride, out_row_stride, B,
                                L, C, stream);
}

extern "C" int osk_residual_add_bf16(const void* a, int64_t a_batch_stride, int64_t a_row_stride, const void* b, int64_t b_batch_stride,
                                     int64_t b_row_stride, void* out, int64_t out_batch_stride, int64_t out_row_stride, int B, int L, int C,
                                     void* stream) {
  return residual_launch<true>(a, a_batch_stride, a_row_stride, b, b_batch_stride, b_row_stride, out, out_batch_stride, out_row_stride,
                                   B, L, C, stream);
}
