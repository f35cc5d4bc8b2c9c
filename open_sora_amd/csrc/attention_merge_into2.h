// The in-place THREE-part merge of osk_attention_merge_into2_bf16 (include/osk.h): kernel and launch, header-only so that the two
// translation units that launch it -- attention_merge.hip (the entry on its own) and attention_fwd.hip (the anchored window entry) --
// share one definition without another symbol between them.
#pragma once
#include "attention_params.h"
#include "../../include/osk.h"

namespace osk_attn {

// In-place THREE-part merge: attn_merge_into_kernel with a second f32 partial (o_c, lse_c -- laid out and indexed as p.ws_o / p.ws_lse,
// the same lse multiplier), folded into the finished rows in the same pass: per (b, l, h) what attn_parts_merge_kernel<3> computes, f32
// sums and ONE rounding, where two passes of the kernel above round twice.  Same grid, same phases; phase 2 loads out_A (one uint4) and
// 32 bytes of each partial (four float4), all in flight before the first use.
// HBM traffic per element of [B, Lq, H * hd]: 2 (out_A read) + 4 (o_B) + 4 (o_C) + 2 (out_A write) = 12 bytes, against 16 for two passes.
template <int HD>
__global__ void __launch_bounds__(256) attn_merge_into2_kernel(const AttnParams p, const float* __restrict__ o_c,
                                                               const float* __restrict__ lse_c, float lse_mult) {
  constexpr int CPR = HD / 8;
  __shared__ float wa[64], wb[64], wc[64];
  const int nqb = (p.Lq + p.rows - 1) / p.rows;
  const int unit = blockIdx.x;
  int bh, qb;
  if (p.map == OSK_ATTN_ORDER_PLAIN) {
    bh = unit / nqb;
    qb = unit - bh * nqb;
  } else {
    unit_to_work(p, nqb, unit, bh, qb);
  }
  const int b = bh / p.H, h = bh - b * p.H;
  const int r0 = blockIdx.y * 64;
  const int row0 = qb * p.rows + r0;
  if (row0 >= p.Lq) return;                                  // (block-uniform)
  const int nrows = p.Lq - row0 < 64 ? p.Lq - row0 : 64;
  const int64_t slot0 = (int64_t)unit * p.rows + r0;
  if ((int)threadIdx.x < nrows) {
    const int64_t at = (int64_t)bh * p.Lq + row0 + threadIdx.x;
    const float la = p.lse[at], lb = p.ws_lse[slot0 + threadIdx.x] * lse_mult, lc = lse_c[slot0 + threadIdx.x] * lse_mult;
    const float m = fmaxf(la, fmaxf(lb, lc));
    const float ea = la == -INFINITY ? 0.f : expf(la - m), eb = lb == -INFINITY ? 0.f : expf(lb - m),
                ec = lc == -INFINITY ? 0.f : expf(lc - m);                                               // (no inf - inf)
    const float tot = ea + eb + ec, inv = tot > 0.f ? 1.0f / tot : 0.f;                                  // all empty: zeros, not NaN
    wa[threadIdx.x] = ea * inv;
    wb[threadIdx.x] = eb * inv;
    wc[threadIdx.x] = ec * inv;
    p.lse[at] = tot > 0.f ? m + logf(tot) : -INFINITY;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < nrows * CPR; i += 256) {
    const int r = i / CPR, c = i - r * CPR;
    unsigned short* po = p.out + b * p.obs + (int64_t)(row0 + r) * p.ors + h * HD + c * 8;
    const float* pb = p.ws_o + (slot0 + r) * HD + c * 8;
    const float* pc = o_c + (slot0 + r) * HD + c * 8;
    const uint4 va = *reinterpret_cast<const uint4*>(po);
    const float4 b0 = *reinterpret_cast<const float4*>(pb), b1 = *reinterpret_cast<const float4*>(pb + 4);
    const float4 c0 = *reinterpret_cast<const float4*>(pc), c1 = *reinterpret_cast<const float4*>(pc + 4);
    const float fb[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
    const float fc[8] = {c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, c1.z, c1.w};
    const float a = wa[r], w = wb[r], u = wc[r];
    float f[8];
    unpack8(va, f);
#pragma unroll
    for (int j = 0; j < 8; ++j)   // (a part without mass may hold anything)
      f[j] = (a > 0.f ? a * f[j] : 0.f) + (w > 0.f ? w * fb[j] : 0.f) + (u > 0.f ? u * fc[j] : 0.f);
    *reinterpret_cast<uint4*>(po) = pack8(f);
  }
}

static inline int launch_merge_into2(const AttnParams& p, const float* o_c, const float* lse_c, int hd, float lse_mult, hipStream_t st) {
  dim3 grid((unsigned)attn_units(p), (unsigned)(p.rows / 64)), block(256);
  if (hd == 64) hipLaunchKernelGGL(attn_merge_into2_kernel<64>, grid, block, 0, st, p, o_c, lse_c, lse_mult);
  else if (hd == 72) hipLaunchKernelGGL(attn_merge_into2_kernel<72>, grid, block, 0, st, p, o_c, lse_c, lse_mult);
  else if (hd == 128) hipLaunchKernelGGL(attn_merge_into2_kernel<128>, grid, block, 0, st, p, o_c, lse_c, lse_mult);
  else return OSK_EUNSUPPORTED;
  return (int)hipGetLastError();
}

}  // namespace osk_attn
