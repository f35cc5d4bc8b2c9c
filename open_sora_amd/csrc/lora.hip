// LoRA merge for gfx950: W' = bf16( W + sum_i scale_i * B_i A_i ), the plan-time step behind open_sora_amd/lora.py
// (include/osk.h, osk_lora_merge_bf16).
//
// One workgroup (4 waves) owns a 128 (n) x 128 (k) tile of the output.  The rank is the MFMA K dimension: per adapter the rank is
// walked in chunks of 32 (zero-padded in LDS, so any 1 <= r <= 256 works), each chunk staged once per workgroup:
//   sA[k][j] = A[j0 + j][k0 + k]   (transposed on the way in: the MFMA wants 8 consecutive ranks per lane)
//   sB[n][j] = B[n0 + n][j0 + j]
// and multiplied on v_mfma_f32_16x16x32_bf16 with the output TRANSPOSED (MFMA rows = k, MFMA columns = n): a lane then owns four
// consecutive k of one weight row per accumulator, and with the row map below two accumulators give it 8 consecutive k -- the 16
// bytes it loads from W and stores to W'.
//   MFMA row rho of tile (g, t)  <->  k = 32 g + 8 (rho >> 2) + 4 t + (rho & 3)          g = 0..3, t = 0..1
//   C/D layout: column = lane & 15, row = 4 (lane >> 4) + reg  ->  k = 32 g + 8 (lane >> 4) + 4 t + reg
// bf16 x bf16 products are exact in f32; every adapter accumulates into its own zero-initialised f32 accumulators, which are added
// to the running f32 sum with one fma by the adapter's scale; W enters that sum last and the result is rounded to bf16 once.
// The kernel streams W once and writes W' once (A and B are re-read from cache by every workgroup): HBM-bound.
#include "osk_common.h"
#include "../../include/osk.h"

#include <cmath>

typedef float f32x4v __attribute__((ext_vector_type(4)));

#define LORA_TN 128         // output rows (n) per workgroup
#define LORA_TK 128         // output columns (k) per workgroup
#define LORA_RC 32          // ranks per staged chunk = the K of one MFMA
#define LORA_LD 40          // LDS row pitch in bf16 (80 bytes: 16-byte aligned fragments, rows spread over the banks)
#define LORA_MAX_ADAPTERS 8
#define LORA_MAX_RANK 256

struct LoraArgs {
  const unsigned short* a[LORA_MAX_ADAPTERS];
  const unsigned short* b[LORA_MAX_ADAPTERS];
  int64_t a_stride[LORA_MAX_ADAPTERS];
  int64_t b_stride[LORA_MAX_ADAPTERS];
  int r[LORA_MAX_ADAPTERS];
  float scale[LORA_MAX_ADAPTERS];
  int n_adapters;
};

__global__ __launch_bounds__(256) void lora_merge_kernel(const unsigned short* w, int64_t w_stride, unsigned short* out,
                                                         int64_t out_stride, int N, int K, LoraArgs args) {
  // (`out` may alias `w`: every element is read and written by the same lane, read first -- no __restrict__ here)
  __shared__ __attribute__((aligned(16))) unsigned short sA[LORA_TK * LORA_LD];
  __shared__ __attribute__((aligned(16))) unsigned short sB[LORA_TN * LORA_LD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int k0 = blockIdx.x * LORA_TK, n0 = blockIdx.y * LORA_TN;
  const int lc = lane & 15, lq = lane >> 4;

  // this lane's 16-byte pieces: rows n0 + 32 wave + 16 cb + lc, columns k0 + 32 g + 8 lq .. + 7
  uint4 wv[2][4];
  bool live[2][4];
#pragma unroll
  for (int cb = 0; cb < 2; ++cb) {
    const int n = n0 + wave * 32 + cb * 16 + lc;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int k = k0 + g * 32 + lq * 8;
      live[cb][g] = n < N && k < K;       // K % 8 == 0: a piece is inside or outside as a whole
      wv[cb][g] = live[cb][g] ? *reinterpret_cast<const uint4*>(w + (int64_t)n * w_stride + k) : make_uint4(0, 0, 0, 0);
    }
  }
  if (args.n_adapters == 0) {             // strided copy, bit for bit
#pragma unroll
    for (int cb = 0; cb < 2; ++cb) {
      const int n = n0 + wave * 32 + cb * 16 + lc;
#pragma unroll
      for (int g = 0; g < 4; ++g)
        if (live[cb][g]) *reinterpret_cast<uint4*>(out + (int64_t)n * out_stride + k0 + g * 32 + lq * 8) = wv[cb][g];
    }
    return;
  }

  f32x4v tot[2][4][2];
#pragma unroll
  for (int cb = 0; cb < 2; ++cb)
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
      for (int t = 0; t < 2; ++t) tot[cb][g][t] = f32x4v{0.f, 0.f, 0.f, 0.f};

  for (int ad = 0; ad < args.n_adapters; ++ad) {
    const unsigned short* A = args.a[ad];
    const unsigned short* B = args.b[ad];
    const int64_t as = args.a_stride[ad], bs = args.b_stride[ad];
    const int r = args.r[ad];
    const bool b_vec = ((bs & 7) == 0) && ((reinterpret_cast<uintptr_t>(B) & 15) == 0);
    f32x4v acc[2][4][2];
#pragma unroll
    for (int cb = 0; cb < 2; ++cb)
#pragma unroll
      for (int g = 0; g < 4; ++g)
#pragma unroll
        for (int t = 0; t < 2; ++t) acc[cb][g][t] = f32x4v{0.f, 0.f, 0.f, 0.f};

    for (int j0 = 0; j0 < r; j0 += LORA_RC) {
      __syncthreads();                    // the previous chunk's fragments have been read
      // A chunk, transposed: 32 ranks x 16 pieces of 8 k = 512 pieces, two per thread
#pragma unroll
      for (int it = 0; it < 2; ++it) {
        const int p = tid + it * 256;
        const int j = p >> 4, c = p & 15;
        const int k = k0 + c * 8;
        uint4 v = make_uint4(0, 0, 0, 0);
        if (j0 + j < r && k < K) v = *reinterpret_cast<const uint4*>(A + (int64_t)(j0 + j) * as + k);
        unsigned short* d = sA + (c * 8) * LORA_LD + j;
        d[0 * LORA_LD] = (unsigned short)(v.x & 0xFFFFu); d[1 * LORA_LD] = (unsigned short)(v.x >> 16);
        d[2 * LORA_LD] = (unsigned short)(v.y & 0xFFFFu); d[3 * LORA_LD] = (unsigned short)(v.y >> 16);
        d[4 * LORA_LD] = (unsigned short)(v.z & 0xFFFFu); d[5 * LORA_LD] = (unsigned short)(v.z >> 16);
        d[6 * LORA_LD] = (unsigned short)(v.w & 0xFFFFu); d[7 * LORA_LD] = (unsigned short)(v.w >> 16);
      }
      // B chunk: 128 rows x 4 pieces of 8 ranks = 512 pieces, two per thread
#pragma unroll
      for (int it = 0; it < 2; ++it) {
        const int p = tid + it * 256;
        const int nl = p >> 2, c = p & 3;
        const int n = n0 + nl, j = j0 + c * 8;
        uint4 v = make_uint4(0, 0, 0, 0);
        if (n < N && j < r) {
          const unsigned short* src = B + (int64_t)n * bs + j;
          if (b_vec && j + 8 <= r) {
            v = *reinterpret_cast<const uint4*>(src);
          } else {                        // rank tail / unaligned rows: element by element, zeros past r
            unsigned e[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) e[i] = (j + i < r) ? (unsigned)src[i] : 0u;
            v = make_uint4(e[0] | (e[1] << 16), e[2] | (e[3] << 16), e[4] | (e[5] << 16), e[6] | (e[7] << 16));
          }
        }
        *reinterpret_cast<uint4*>(sB + nl * LORA_LD + c * 8) = v;
      }
      __syncthreads();
      bf16x8_t bf[2];
#pragma unroll
      for (int cb = 0; cb < 2; ++cb)
        bf[cb] = __builtin_bit_cast(bf16x8_t, *reinterpret_cast<const uint4*>(sB + (wave * 32 + cb * 16 + lc) * LORA_LD + lq * 8));
#pragma unroll
      for (int g = 0; g < 4; ++g)
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          const int krow = g * 32 + (lc >> 2) * 8 + t * 4 + (lc & 3);
          const bf16x8_t af = __builtin_bit_cast(bf16x8_t, *reinterpret_cast<const uint4*>(sA + krow * LORA_LD + lq * 8));
#pragma unroll
          for (int cb = 0; cb < 2; ++cb)
            acc[cb][g][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, bf[cb], acc[cb][g][t], 0, 0, 0);
        }
    }
    const float s = args.scale[ad];
#pragma unroll
    for (int cb = 0; cb < 2; ++cb)
#pragma unroll
      for (int g = 0; g < 4; ++g)
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
          for (int i = 0; i < 4; ++i) tot[cb][g][t][i] = __builtin_fmaf(s, acc[cb][g][t][i], tot[cb][g][t][i]);
  }

#pragma unroll
  for (int cb = 0; cb < 2; ++cb) {
    const int n = n0 + wave * 32 + cb * 16 + lc;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      if (!live[cb][g]) continue;
      float f[8];
      unpack8(wv[cb][g], f);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        f[i] += tot[cb][g][0][i];
        f[4 + i] += tot[cb][g][1][i];
      }
      *reinterpret_cast<uint4*>(out + (int64_t)n * out_stride + k0 + g * 32 + lq * 8) = pack8(f);
    }
  }
}

extern "C" int osk_lora_merge_bf16(const void* w, int64_t w_row_stride, void* out, int64_t out_row_stride, int N, int K,
                                   const OskLoraAdapter* adapters, int n_adapters, void* stream) {
  if (!w || !out || N < 1 || K < 8 || (K & 7)) return OSK_EINVAL;
  if (w_row_stride < K || out_row_stride < K || (w_row_stride & 7) || (out_row_stride & 7)) return OSK_EINVAL;
  if ((reinterpret_cast<uintptr_t>(w) & 15) || (reinterpret_cast<uintptr_t>(out) & 15)) return OSK_EINVAL;
  if (n_adapters < 0 || n_adapters > LORA_MAX_ADAPTERS || (n_adapters > 0 && !adapters)) return OSK_EINVAL;
  if ((int64_t)(N + LORA_TN - 1) / LORA_TN > 65535) return OSK_EINVAL;
  LoraArgs args;
  args.n_adapters = n_adapters;
  for (int i = 0; i < LORA_MAX_ADAPTERS; ++i) {
    args.a[i] = args.b[i] = nullptr;
    args.a_stride[i] = args.b_stride[i] = 0;
    args.r[i] = 0;
    args.scale[i] = 0.f;
  }
  for (int i = 0; i < n_adapters; ++i) {
    const OskLoraAdapter& ad = adapters[i];
    if (!ad.a || !ad.b || ad.r < 1 || ad.r > LORA_MAX_RANK || !std::isfinite(ad.scale)) return OSK_EINVAL;
    if (ad.a_row_stride < K || (ad.a_row_stride & 7) || (reinterpret_cast<uintptr_t>(ad.a) & 15)) return OSK_EINVAL;
    if (ad.b_row_stride < ad.r || (reinterpret_cast<uintptr_t>(ad.b) & 1)) return OSK_EINVAL;
    args.a[i] = static_cast<const unsigned short*>(ad.a);
    args.b[i] = static_cast<const unsigned short*>(ad.b);
    args.a_stride[i] = ad.a_row_stride;
    args.b_stride[i] = ad.b_row_stride;
    args.r[i] = ad.r;
    args.scale[i] = ad.scale;
  }
  const dim3 grid((unsigned)((K + LORA_TK - 1) / LORA_TK), (unsigned)((N + LORA_TN - 1) / LORA_TN));
  hipLaunchKernelGGL(lora_merge_kernel, grid, dim3(256), 0, (hipStream_t)stream, static_cast<const unsigned short*>(w), w_row_stride,
                     static_cast<unsigned short*>(out), out_row_stride, N, K, args);
  return (int)hipGetLastError();
}
