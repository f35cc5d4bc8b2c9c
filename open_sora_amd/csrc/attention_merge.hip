// osk_attention_merge_bf16: combine S attention results over disjoint key sets by their log-sum-exp (include/osk.h).
// The sequence-parallel all-gather cut into S key slices (open_sora_amd/seqpar.py, kv_chunks) runs one flash launch per slice as
// that slice arrives and merges the S (out, lse) pairs here: _rescale_out_lse of opensora/models/mmdit/distributed.py:223-313
// applied once to all parts instead of hop by hop.
//
// Roofline: HBM.  Bytes = (S + 1) * B * L * H * hd * 2 (+ (S + 1) * B * H * L * 4 of lse): every partial row is read once, the
// result written once.  A block owns `rows` consecutive query rows of one batch item.  Phase 1: one thread per (row, head) reads
// that pair's S lse values -- once, not once per element -- and leaves the S normalised weights in LDS.  Phase 2: one thread per
// 16-byte chunk of a row (8 bf16; a chunk never straddles heads because hd % 8 == 0) loads its S partial chunks, all in flight
// before the first use, accumulates in f32 and stores one rounded uint4.  No allocation, no memset, no atomics, no
// synchronisation with the host: capturable in a hipGraph.
#include "osk_common.h"
#include "../../include/osk.h"

namespace {

constexpr int MERGE_MAX_PARTS = 8;
constexpr int MERGE_PAIRS = 512;     // (row, head) pairs of one block: 512 * 8 weights = 16 KiB of LDS

template <int S>
__global__ void __launch_bounds__(256) attn_parts_merge_kernel(const unsigned short* __restrict__ parts, int64_t pps, int64_t pbs, int64_t prs,
                                                               const float* __restrict__ lse, unsigned short* __restrict__ out, int64_t obs,
                                                               int64_t ors, float* __restrict__ lse_out, int B, int H, int L, int hd, int rows) {
  __shared__ __attribute__((aligned(16))) float wn[MERGE_PAIRS * MERGE_MAX_PARTS];
  const int b = blockIdx.y;
  const int64_t l0 = (int64_t)blockIdx.x * rows;
  const int nrows = (int)((L - l0) < rows ? (L - l0) : rows);

  // phase 1: the weights of every (row, head) of the block; consecutive threads = consecutive rows of one head (lse is [.., H, L])
  for (int t = threadIdx.x; t < rows * H; t += 256) {
    const int h = t / rows, r = t - h * rows;
    if (r >= nrows) continue;
    const int64_t at = ((int64_t)b * H + h) * L + l0 + r;
    float l[S], m = -INFINITY;
#pragma unroll
    for (int s = 0; s < S; ++s) {
      l[s] = lse[(int64_t)s * B * H * L + at];
      m = fmaxf(m, l[s]);
    }
    float tot = 0.f;
#pragma unroll
    for (int s = 0; s < S; ++s) {
      l[s] = (l[s] == -INFINITY) ? 0.f : expf(l[s] - m);     // (a part without keys, and m == -inf: no inf - inf)
      tot += l[s];
    }
    const float inv = tot > 0.f ? 1.0f / tot : 0.f;            // every part empty: zeros, not NaN
    float* w = wn + (r * H + h) * MERGE_MAX_PARTS;
#pragma unroll
    for (int s = 0; s < S; ++s) w[s] = l[s] * inv;
    if (lse_out) lse_out[at] = tot > 0.f ? m + logf(tot) : -INFINITY;
  }
  __syncthreads();

  // phase 2: 16-byte chunks of the block's rows
  const int D8 = H * hd / 8;
  const unsigned short* pb = parts + (int64_t)b * pbs;
  unsigned short* ob = out + (int64_t)b * obs;
  for (int i = threadIdx.x; i < nrows * D8; i += 256) {
    const int r = i / D8, c = i - r * D8;
    const int h = c * 8 / hd;
    const int64_t row = l0 + r;
    uint4 v[S];
#pragma unroll
    for (int s = 0; s < S; ++s) v[s] = *reinterpret_cast<const uint4*>(pb + (int64_t)s * pps + row * prs + c * 8);
    const float* w = wn + (r * H + h) * MERGE_MAX_PARTS;
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < S; ++s) {
      float f[8];
      unpack8(v[s], f);
      const float ws = w[s];
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[j] = __builtin_fmaf(ws, f[j], acc[j]);
    }
    *reinterpret_cast<uint4*>(ob + row * ors + c * 8) = pack8(acc);
  }
}

template <int S>
int launch(const void* parts, int64_t pps, int64_t pbs, int64_t prs, const float* lse, void* out, int64_t obs, int64_t ors, float* lse_out,
           int B, int H, int L, int hd, int rows, hipStream_t st) {
  dim3 grid((unsigned)((L + rows - 1) / rows), (unsigned)B), block(256);
  hipLaunchKernelGGL(attn_parts_merge_kernel<S>, grid, block, 0, st, (const unsigned short*)parts, pps, pbs, prs, lse, (unsigned short*)out,
                     obs, ors, lse_out, B, H, L, hd, rows);
  return (int)hipGetLastError();
}

}  // namespace

extern "C" int osk_attention_merge_bf16(const void* parts, int64_t part_stride, int64_t p_batch_stride, int64_t p_row_stride,
                                        const float* lse, void* out, int64_t o_batch_stride, int64_t o_row_stride, float* lse_out,
                                        int S, int B, int H, int L, int hd, void* stream) {
  if (!parts || !lse || !out || S < 1 || S > MERGE_MAX_PARTS || B <= 0 || H <= 0 || L <= 0 || hd <= 0 || (hd & 7)) return OSK_EINVAL;
  if ((part_stride & 7) || (p_batch_stride & 7) || (p_row_stride & 7) || (o_batch_stride & 7) || (o_row_stride & 7)) return OSK_EINVAL;
  if (part_stride < 0 || p_batch_stride < 0 || o_batch_stride < 0 || p_row_stride < (int64_t)H * hd || o_row_stride < (int64_t)H * hd)
    return OSK_EINVAL;
  if (((uintptr_t)parts & 15) || ((uintptr_t)out & 15) || ((uintptr_t)lse & 3) || ((uintptr_t)lse_out & 3)) return OSK_EINVAL;
  if (H > MERGE_PAIRS || B > 65535 || (int64_t)H * hd > (1 << 24)) return OSK_EUNSUPPORTED;
  const int rows = MERGE_PAIRS / H < 8 ? MERGE_PAIRS / H : 8;
  hipStream_t st = (hipStream_t)stream;
#define OSK_MERGE_CASE(N) \
  case N: return launch<N>(parts, part_stride, p_batch_stride, p_row_stride, lse, out, o_batch_stride, o_row_stride, lse_out, B, H, L, hd, rows, st)
  switch (S) {
    OSK_MERGE_CASE(1);
    OSK_MERGE_CASE(2);
    OSK_MERGE_CASE(3);
    OSK_MERGE_CASE(4);
    OSK_MERGE_CASE(5);
    OSK_MERGE_CASE(6);
    OSK_MERGE_CASE(7);
    OSK_MERGE_CASE(8);
  }
#undef OSK_MERGE_CASE
  return OSK_EINVAL;
}
