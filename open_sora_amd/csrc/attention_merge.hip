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
//
// osk_attention_merge_into_bf16 (attn_merge_into_kernel below): the two-part form that updates one finished (out, lse) pair IN
// PLACE from the f32 partial of a second launch over other keys -- the last-segment launch of osk_attention_fwd_ragged_bf16.
// osk_attention_merge_into2_bf16 (attn_merge_into2_kernel, attention_merge_into2.h): the same with TWO partials in one pass -- the prefix and suffix launches
// of osk_attention_fwd_window_anchor_bf16.
#include "attention_params.h"
#include "attention_merge_into2.h"
#include "../../include/osk.h"

using osk_attn::AttnParams;

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

// In-place two-part merge.  grid (work units of the partial's launch, rows per unit / 64): a block owns 64 query rows of one (batch,
// head).  Phase 1: thread r reads lse_A and lse_B of row r -- once per (row, head) --, leaves the two normalised weights in LDS and
// writes the merged lse over lse_A (nobody else reads that value).  Phase 2: one thread per 16-byte chunk of an output row (8 bf16;
// hd % 8 == 0) loads out_A (one uint4) and the matching 32 bytes of the f32 partial (two float4), combines in f32 and stores the
// rounded uint4 where it read out_A.  Rows >= Lq are neither read nor written; no third image of the rows exists.
// HBM traffic per element of [B, Lq, H * hd]: 2 (out_A read) + 4 (o_B read) + 2 (out_A write) = 8 bytes (+ 12 bytes of lse per (row, head)).
template <int HD>
__global__ void __launch_bounds__(256) attn_merge_into_kernel(const AttnParams p, float lse_b_mult) {
  constexpr int CPR = HD / 8;
  __shared__ float wa[64], wb[64];
  const int nqb = (p.Lq + p.rows - 1) / p.rows;
  const int unit = blockIdx.x;
  int bh, qb;
  if (p.map == OSK_ATTN_ORDER_PLAIN) {
    bh = unit / nqb;
    qb = unit - bh * nqb;
  } else {
    osk_attn::unit_to_work(p, nqb, unit, bh, qb);
  }
  const int b = bh / p.H, h = bh - b * p.H;
  const int r0 = blockIdx.y * 64;
  const int row0 = qb * p.rows + r0;
  if (row0 >= p.Lq) return;                                  // (block-uniform)
  const int nrows = p.Lq - row0 < 64 ? p.Lq - row0 : 64;
  const int64_t slot0 = (int64_t)unit * p.rows + r0;
  if ((int)threadIdx.x < nrows) {
    const int64_t at = (int64_t)bh * p.Lq + row0 + threadIdx.x;
    const float la = p.lse[at], lb = p.ws_lse[slot0 + threadIdx.x] * lse_b_mult;
    const float m = fmaxf(la, lb);
    const float ea = la == -INFINITY ? 0.f : expf(la - m), eb = lb == -INFINITY ? 0.f : expf(lb - m);   // (no inf - inf)
    const float tot = ea + eb, inv = tot > 0.f ? 1.0f / tot : 0.f;                                       // both empty: zeros, not NaN
    wa[threadIdx.x] = ea * inv;
    wb[threadIdx.x] = eb * inv;
    p.lse[at] = tot > 0.f ? m + logf(tot) : -INFINITY;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < nrows * CPR; i += 256) {
    const int r = i / CPR, c = i - r * CPR;
    unsigned short* po = p.out + b * p.obs + (int64_t)(row0 + r) * p.ors + h * HD + c * 8;
    const float* pb = p.ws_o + (slot0 + r) * HD + c * 8;
    const uint4 va = *reinterpret_cast<const uint4*>(po);
    const float4 b0 = *reinterpret_cast<const float4*>(pb), b1 = *reinterpret_cast<const float4*>(pb + 4);
    const float fb[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
    const float a = wa[r], w = wb[r];
    float f[8];
    unpack8(va, f);
#pragma unroll
    for (int j = 0; j < 8; ++j) f[j] = (a > 0.f ? a * f[j] : 0.f) + (w > 0.f ? w * fb[j] : 0.f);   // (a part without mass may hold anything)
    *reinterpret_cast<uint4*>(po) = pack8(f);
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

int osk_attn::launch_merge_into(const AttnParams& p, int hd, float lse_b_mult, hipStream_t st) {
  dim3 grid((unsigned)attn_units(p), (unsigned)(p.rows / 64)), block(256);
  if (hd == 64) hipLaunchKernelGGL(attn_merge_into_kernel<64>, grid, block, 0, st, p, lse_b_mult);
  else if (hd == 72) hipLaunchKernelGGL(attn_merge_into_kernel<72>, grid, block, 0, st, p, lse_b_mult);
  else if (hd == 128) hipLaunchKernelGGL(attn_merge_into_kernel<128>, grid, block, 0, st, p, lse_b_mult);
  else return OSK_EUNSUPPORTED;
  return (int)hipGetLastError();
}

extern "C" int osk_attention_merge_into_bf16(void* out, int64_t o_batch_stride, int64_t o_row_stride, float* lse, const float* o_b,
                                             const float* lse_b, int B, int H, int Lq, int hd, void* stream) {
  if (!out || !lse || !o_b || !lse_b || B <= 0 || H <= 0 || Lq <= 0) return OSK_EINVAL;
  if ((o_batch_stride & 7) || (o_row_stride & 7) || o_batch_stride < 0 || o_row_stride < (int64_t)H * hd) return OSK_EINVAL;
  if (((uintptr_t)out & 15) || ((uintptr_t)o_b & 15) || ((uintptr_t)lse & 3) || ((uintptr_t)lse_b & 3)) return OSK_EINVAL;
  if (hd != 64 && hd != 72 && hd != 128) return OSK_EUNSUPPORTED;
  AttnParams p{};
  p.out = (unsigned short*)out; p.obs = o_batch_stride; p.ors = o_row_stride;
  p.lse = lse; p.B = B; p.H = H; p.Lq = Lq;
  p.rows = 256;
  p.map = OSK_ATTN_ORDER_PLAIN;
  p.ws_o = const_cast<float*>(o_b); p.ws_lse = const_cast<float*>(lse_b);
  return osk_attn::launch_merge_into(p, hd, 1.0f, (hipStream_t)stream);
}

extern "C" int osk_attention_merge_into2_bf16(void* out, int64_t o_batch_stride, int64_t o_row_stride, float* lse, const float* o_b,
                                              const float* lse_b, const float* o_c, const float* lse_c, int B, int H, int Lq, int hd,
                                              void* stream) {
  if (!out || !lse || !o_b || !lse_b || !o_c || !lse_c || B <= 0 || H <= 0 || Lq <= 0) return OSK_EINVAL;
  if ((o_batch_stride & 7) || (o_row_stride & 7) || o_batch_stride < 0 || o_row_stride < (int64_t)H * hd) return OSK_EINVAL;
  if (((uintptr_t)out & 15) || ((uintptr_t)o_b & 15) || ((uintptr_t)o_c & 15) || ((uintptr_t)lse & 3) || ((uintptr_t)lse_b & 3) ||
      ((uintptr_t)lse_c & 3))
    return OSK_EINVAL;
  if (hd != 64 && hd != 72 && hd != 128) return OSK_EUNSUPPORTED;
  AttnParams p{};
  p.out = (unsigned short*)out; p.obs = o_batch_stride; p.ors = o_row_stride;
  p.lse = lse; p.B = B; p.H = H; p.Lq = Lq;
  p.rows = 256;
  p.map = OSK_ATTN_ORDER_PLAIN;
  p.ws_o = const_cast<float*>(o_b); p.ws_lse = const_cast<float*>(lse_b);
  return osk_attn::launch_merge_into2(p, o_c, lse_c, hd, 1.0f, (hipStream_t)stream);
}

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
