// Entry points of the flash-attention family (bf16 in / out, f32 softmax, non-causal) + the tail-split merge kernel + the fp8
// V^T preparation.  The kernels themselves are the hand-scheduled, generated loops of attention_asm72.hip (head_dim 72 and, on the
// same loop with zero dims 64..71, head_dim 64), attention_asm72w.hip (their wide layout for bounded calls with >= 1024 query
// rows), attention_asm128.hip and the fp8 P.V variants.  Round 4 removed the last compiler-scheduled flash kernel
// (attn_fwd_kernel<64>, 400 lines: 8 waves x 32 rows, register-staged tiles) -- head_dim 64 now runs the head_dim-72 loop.
//
// Roofline: MFMA bf16.  Algorithmic FLOPs = 4 * B * H * Lq * Lk * hd (QK^T + PV, not halved).
#include <algorithm>
#include <atomic>
#include <initializer_list>
#include "attention_params.h"
#include "attention_merge_into2.h"
#include "../../include/osk.h"

using osk_attn::AttnParams;

namespace osk_attn {
namespace {

// combine the key parts of the split tail units: out = sum_p 2^(lse_p - lse) O_p, lse = log2 sum_p 2^lse_p.
// grid (tail units, 4): a block owns 64 query rows; thread = (row, 16-byte chunk of the head dim), so the partial rows
// -- contiguous [row][hd] f32 in the workspace -- are read as one linear stream per part.  A few tens of MB in all.
template <int HD>
__global__ void __launch_bounds__(256) attn_merge_kernel(const AttnParams p) {
  constexpr int CPR = HD / 4;                    // float4 chunks per row
  const int nqb = (p.Lq + p.rows - 1) / p.rows;
  int bh, qb;
  unit_to_work(p, nqb, p.tail_first + (int)blockIdx.x, bh, qb);
  const int b = bh / p.H, h = bh - b * p.H;
  float bound_;
  if (!attn_auto_bound(p, b, h, true, bound_)) return;   // auto-dispatched pair: this unit was the general twin's (it writes final rows itself)
  const int S = p.tail_split;
  for (int i = threadIdx.x; i < 64 * CPR; i += 256) {
    const int r = blockIdx.y * 64 + i / CPR, c = i % CPR;
    const int row = qb * p.rows + r;
    if (row >= p.Lq) continue;
    const int64_t slot0 = (int64_t)blockIdx.x * S * p.rows + r;
    float l[8], m = -INFINITY;
    for (int s = 0; s < S; ++s) { l[s] = p.ws_lse[slot0 + s * p.rows]; m = fmaxf(m, l[s]); }
    float tot = 0.f;
    for (int s = 0; s < S; ++s) { l[s] = exp2f(l[s] - m); tot += l[s]; }
    const float inv = 1.0f / tot;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int s = 0; s < S; ++s) {
      const float4 v = *reinterpret_cast<const float4*>(p.ws_o + (slot0 + (int64_t)s * p.rows) * HD + c * 4);
      acc.x += l[s] * v.x; acc.y += l[s] * v.y; acc.z += l[s] * v.z; acc.w += l[s] * v.w;
    }
    uint2 w2;
    w2.x = pack_bf16x2(acc.x * inv, acc.y * inv);
    w2.y = pack_bf16x2(acc.z * inv, acc.w * inv);
    *reinterpret_cast<uint2*>(p.out + b * p.obs + (int64_t)row * p.ors + h * HD + c * 4) = w2;
    if (p.lse && c == 0) p.lse[(int64_t)bh * p.Lq + row] = (m + log2f(tot)) * 0.6931471805599453f;
  }
}

}  // namespace

// A workgroup owns a CU for its whole key loop, so a launch takes ceil(units / CUs) rounds and the last round may run
// a fraction of the chip (3168 units on 256 CUs: 12.4 -> 13; sequence-parallel ranks: 1.7 -> 2, 3.2 -> 4).  With a
// workspace the units of that last round are cut into `s` key parts (whole key segments when there are several,
// else runs of 64-key tiles) so that the round costs ceil(R s / CUs) / s instead of 1; only those units pay the
// partial-result traffic.  s <= 8, chosen to minimise that cost; no split when it saves < 15 % of a round.
void split_tail(AttnParams& p, int units, int hd, void* workspace, int64_t workspace_bytes) {
  p.tail_split = 1;
  p.tail_first = 0x7fffffff;
  if (!workspace || p.win) return;   // (a windowed launch: its units have key runs of their own)
  const int cus = osk_device_cus();
  const int R = units % cus;
  if (R == 0) return;
  auto cost = [&](int s) { return (double)((R * s + cus - 1) / cus) / s; };
  int best = 1;
  for (int s = 2; s <= 8; ++s) {
    if (p.n_seg > 1 ? (p.n_seg % s != 0) : (s > p.tps)) continue;
    const int64_t need = (int64_t)R * s * p.rows * (hd + 1) * 4;
    if (need > workspace_bytes) continue;
    if (cost(s) < cost(best) - 1e-9) best = s;
  }
  if (cost(1) - cost(best) < 0.15) return;
  p.tail_split = best;
  p.tail_first = units - R;
  p.ws_o = (float*)workspace;
  p.ws_lse = p.ws_o + (int64_t)R * best * p.rows * hd;
}

int launch_merge(const AttnParams& p, int hd, hipStream_t st) {
  dim3 grid(attn_units(p) - p.tail_first, p.rows / 64), block(256);
  if (hd == 72) hipLaunchKernelGGL(attn_merge_kernel<72>, grid, block, 0, st, p);
  else if (hd == 64) hipLaunchKernelGGL(attn_merge_kernel<64>, grid, block, 0, st, p);
  else if (hd == 128) hipLaunchKernelGGL(attn_merge_kernel<128>, grid, block, 0, st, p);
  else return OSK_EUNSUPPORTED;
  return (int)hipGetLastError();
}

}  // namespace osk_attn

// reporting: (key parts, rows per work unit) the launch of a call with these arguments uses -- the SAME selection code as
// osk_attention_fwd_bounded_bf16 below (round 4 modelled 256-row units whatever the call: ADVICE r4)
static std::atomic<int> g_rows_override{0};   // tools only (osk_attention_rows_override): 0 = by estimate, 256 / 512 = forced where legal
static void launch_shape(AttnParams& p, int hd, void* workspace, int64_t workspace_bytes) {
  p.rows = 256;
  const int forced = g_rows_override.load(std::memory_order_relaxed);
  const bool wide_legal = (hd == 72 || hd == 64) && osk_attn::attn_fast_path(p) && p.Lq >= 1024;
  if (forced ? (forced == 512 && wide_legal) : osk_attn::attn_wide_path(p, hd, osk_device_cus(), workspace != nullptr)) p.rows = 512;
  if (hd == 64 || hd == 72 || hd == 128) osk_attn::split_tail(p, osk_attn::attn_units(p), hd, workspace, workspace_bytes);
}

static void set_segments(AttnParams& p, int n_seg, int seg_len) {
  p.n_seg = n_seg; p.seg_len = seg_len;
  p.seg_lp = (seg_len + 63) / 64 * 64;
  p.tps = p.seg_lp / 64;
}

static float bound_to_bf16_up(float score_bound) {
  // the kernels keep the bound in a bf16 field of Q's padding dim: round it UP to the next bf16 value (it stays a bound)
  const unsigned bits = __builtin_bit_cast(unsigned, score_bound);
  return __builtin_bit_cast(float, (bits + 0xFFFFu) & 0xFFFF0000u);
}

extern "C" int osk_attention_launch_shape(int B, int H, int Lq, int n_seg, int seg_len, int hd, float score_bound,
                                          int64_t workspace_bytes, int* rows_per_unit) {
  if (rows_per_unit) *rows_per_unit = 256;
  if (B <= 0 || H <= 0 || Lq <= 0 || n_seg <= 0 || seg_len <= 0 || (hd != 64 && hd != 72 && hd != 128) || !(score_bound >= 0.f)) return 1;
  AttnParams p{};
  p.B = B; p.H = H; p.Lq = Lq;
  set_segments(p, n_seg, seg_len);
  p.bound = bound_to_bf16_up(score_bound);
  static char dummy[16] __attribute__((aligned(16)));
  launch_shape(p, hd, workspace_bytes > 0 ? dummy : nullptr, workspace_bytes);
  if (rows_per_unit) *rows_per_unit = p.rows;
  return p.tail_split;
}

extern "C" int osk_attention_rows_override(int rows_per_unit) {
  if (rows_per_unit != 0 && rows_per_unit != 256 && rows_per_unit != 512) return OSK_EINVAL;
  g_rows_override.store(rows_per_unit, std::memory_order_relaxed);
  return OSK_OK;
}

extern "C" int osk_attention_tail_split_factor(int B, int H, int Lq, int n_seg, int seg_len, int hd,
                                               int64_t workspace_bytes) {
  return osk_attention_launch_shape(B, H, Lq, n_seg, seg_len, hd, 0.0f, workspace_bytes, nullptr);
}

extern "C" int64_t osk_attention_workspace_bytes(void) {
  // enough for 512 key parts (two rounds of a 256-CU chip) of 256 rows at head_dim 128: partial O + LSE in f32
  return (int64_t)512 * 256 * (128 + 1) * 4;
}

extern "C" int osk_attention_fwd_bf16(const void* q, int64_t q_batch_stride, int64_t q_row_stride,
                                      const void* k, int64_t k_seg_stride, int64_t k_batch_stride,
                                      int64_t k_row_stride, const void* vt, int64_t vt_seg_stride,
                                      void* out, int64_t o_batch_stride, int64_t o_row_stride,
                                      float* lse, int B, int H, int Lq, int n_seg, int seg_len, int hd,
                                      float scale, int q_prescaled, int kv_batches, void* stream) {
  return osk_attention_fwd_ws_bf16(q, q_batch_stride, q_row_stride, k, k_seg_stride, k_batch_stride, k_row_stride, vt,
                                   vt_seg_stride, out, o_batch_stride, o_row_stride, lse, B, H, Lq, n_seg, seg_len, hd,
                                   scale, q_prescaled, kv_batches, nullptr, 0, stream);
}

// The argument checks and the AttnParams fill the three entry points share.  What differs between them is an argument: vt_stride_mask (7:
// bf16 V^T, strides in elements; 15: the e4m3 layout of the pv8 variant, its stride in bytes) and hds, the head dims the entry point has
// kernels for.  Status precedence: OSK_EINVAL before OSK_EUNSUPPORTED -- an entry point makes its own OSK_EINVAL checks before it calls this
// function and its own OSK_EUNSUPPORTED checks after it, so a malformed call is reported as malformed whatever head dim it asks for.
static int attn_params(AttnParams& p, const void* q, int64_t q_batch_stride, int64_t q_row_stride, const void* k, int64_t k_seg_stride,
                       int64_t k_batch_stride, int64_t k_row_stride, const void* vt, int64_t vt_seg_stride, int64_t vt_stride_mask,
                       void* out, int64_t o_batch_stride, int64_t o_row_stride, float* lse, int B, int H, int Lq, int n_seg, int seg_len,
                       int hd, std::initializer_list<int> hds, float scale, int q_prescaled, int kv_batches, const void* workspace,
                       int64_t workspace_bytes) {
  if (!q || !k || !vt || !out || B <= 0 || H <= 0 || Lq <= 0 || n_seg <= 0 || seg_len <= 0) return OSK_EINVAL;
  if ((q_batch_stride & 7) || (q_row_stride & 7) || (k_seg_stride & 7) || (k_batch_stride & 7) || (k_row_stride & 7) ||
      (vt_seg_stride & vt_stride_mask) || (o_batch_stride & 3) || (o_row_stride & 3))
    return OSK_EINVAL;
  if (((uintptr_t)q & 15) || ((uintptr_t)k & 15) || ((uintptr_t)vt & 15) || ((uintptr_t)out & 7)) return OSK_EINVAL;
  if (kv_batches < 0 || kv_batches > B) return OSK_EINVAL;
  if (workspace && (((uintptr_t)workspace & 15) || workspace_bytes < 0)) return OSK_EINVAL;
  if (std::find(hds.begin(), hds.end(), hd) == hds.end()) return OSK_EUNSUPPORTED;
  p.q = (const unsigned short*)q; p.qbs = q_batch_stride; p.qrs = q_row_stride;
  p.k = (const unsigned short*)k; p.kss = k_seg_stride; p.kbs = k_batch_stride; p.krs = k_row_stride;
  p.vt = (const unsigned short*)vt; p.vtss = vt_seg_stride;
  p.out = (unsigned short*)out; p.obs = o_batch_stride; p.ors = o_row_stride;
  p.lse = lse; p.B = B; p.H = H; p.Lq = Lq;
  set_segments(p, n_seg, seg_len);
  p.sc = q_prescaled ? 1.0f : scale * 1.4426950408889634f;  // log2 units; 1: q already carries it
  p.q_prescaled = q_prescaled;
  p.Bkv = kv_batches > 0 ? kv_batches : B;
  p.map = 1;   // XCD-contiguous work order (each XCD walks one head's K / V^T stream)
  return OSK_OK;
}

// ONE kernel per (head_dim, query rows per work unit); the FAST / general body is the launch function's choice (attn_fast_path)
static int run(const AttnParams& p, int hd, hipStream_t st) {
  const bool wide = p.rows == 512;
  switch (hd) {
    case 64: return wide ? osk_attn::launch_asm64w(p, st) : osk_attn::launch_asm64(p, st);
    case 72: return wide ? osk_attn::launch_asm72w(p, st) : osk_attn::launch_asm72(p, st);
    case 128: return osk_attn::launch_asm128(p, st);
    default: return OSK_EUNSUPPORTED;
  }
}

// after a launch that returned rc: combine the key parts of its split tail units (launch_shape / split_tail decided whether there are any)
static int then_merge(int rc, const AttnParams& p, int hd, hipStream_t st) {
  return rc != 0 || p.tail_split == 1 ? rc : osk_attn::launch_merge(p, hd, st);
}

// The kernel family of a filled parameter block (OSK_ATTN_* of include/osk.h): bf16 operands (p.bound set), e4m3 V^T, e4m3 K and V^T
static int run_mode(const AttnParams& p, int hd, int mode, hipStream_t st) {
  if (mode == OSK_ATTN_BF16) return run(p, hd, st);
  if (mode == OSK_ATTN_QK8) return osk_attn::launch_asm128q8(p, st);
  return hd == 128 ? osk_attn::launch_asm128p8(p, st) : osk_attn::launch_asm72p8(p, st);
}

// One call of an entry point on a filled parameter block: launch shape, kernel, merge of the split tail units
static int dispatch(AttnParams& p, int hd, int mode, void* workspace, int64_t workspace_bytes, hipStream_t st) {
  if (mode == OSK_ATTN_BF16) launch_shape(p, hd, workspace, workspace_bytes);
  else osk_attn::split_tail(p, osk_attn::attn_units(p), hd, workspace, workspace_bytes);
  return then_merge(run_mode(p, hd, mode, st), p, hd, st);
}

// The operands of a call by mode (OSK_ATTN_* of include/osk.h), in front of attn_params(): the mode's OSK_EINVAL checks, attn_params() with
// the mode's V^T stride mask (7: bf16, elements; 15: e4m3, bytes) and head dims, the mode's OSK_EUNSUPPORTED check, then K and V^T retagged
// as the kernel family reads them and the bound set.  k_scale / v_scale of another mode are ignored; score_bound is checked in every mode
// and used in OSK_ATTN_BF16 (an entry without one passes 0).  v_scale_mask: 3, the alignment of an f32 vector -- osk_attention_fwd_pv8_bf16
// alone has never checked it and passes 0.  Status precedence as attn_params states it: an entry makes its own OSK_EINVAL checks first.
static int mode_params(AttnParams& p, int mode, const float* k_scale, const float* v_scale, uintptr_t v_scale_mask, float score_bound,
                       const void* q, int64_t q_batch_stride, int64_t q_row_stride, const void* k, int64_t k_seg_stride,
                       int64_t k_batch_stride, int64_t k_row_stride, const void* vt, int64_t vt_seg_stride, void* out,
                       int64_t o_batch_stride, int64_t o_row_stride, float* lse, int B, int H, int Lq, int n_seg, int seg_len, int hd,
                       float scale, int q_prescaled, int kv_batches, const void* workspace, int64_t workspace_bytes) {
  using hds = std::initializer_list<int>;
  if (mode != OSK_ATTN_BF16 && mode != OSK_ATTN_PV8 && mode != OSK_ATTN_QK8) return OSK_EINVAL;
  if (!(score_bound >= 0.f)) return OSK_EINVAL;   // (also rejects NaN)
  if (mode != OSK_ATTN_BF16 && (!v_scale || ((uintptr_t)v_scale & v_scale_mask))) return OSK_EINVAL;
  if (mode == OSK_ATTN_QK8 && (!k_scale || ((uintptr_t)k_scale & 3) || (k_seg_stride & 15) || (k_batch_stride & 15) || k_seg_stride < 0 ||
                               k_batch_stride < 0))
    return OSK_EINVAL;
  const int rc = attn_params(p, q, q_batch_stride, q_row_stride, k, k_seg_stride, k_batch_stride, k_row_stride, vt, vt_seg_stride,
                             mode == OSK_ATTN_BF16 ? 7 : 15, out, o_batch_stride, o_row_stride, lse, B, H, Lq, n_seg, seg_len, hd,
                             mode == OSK_ATTN_BF16 ? hds{64, 72, 128} : mode == OSK_ATTN_PV8 ? hds{72, 128} : hds{128}, scale, q_prescaled,
                             kv_batches, workspace, workspace_bytes);
  if (rc != OSK_OK) return rc;
  if (mode == OSK_ATTN_QK8 && k_row_stride != 128) return OSK_EUNSUPPORTED;   // the packed layout: rows of 128 bytes, heads seg_lp rows apart
  if (mode == OSK_ATTN_BF16) {
    p.bound = bound_to_bf16_up(score_bound);
  } else {
    p.vt = nullptr; p.vt8 = (const unsigned char*)vt; p.v_scale = v_scale;
    if (mode == OSK_ATTN_QK8) { p.k = nullptr; p.k8 = (const unsigned char*)k; p.k_scale = k_scale; }
  }
  return OSK_OK;
}

extern "C" int osk_attention_fwd_bounded_bf16(const void* q, int64_t q_batch_stride, int64_t q_row_stride,
                                         const void* k, int64_t k_seg_stride, int64_t k_batch_stride,
                                         int64_t k_row_stride, const void* vt, int64_t vt_seg_stride,
                                         void* out, int64_t o_batch_stride, int64_t o_row_stride,
                                         float* lse, int B, int H, int Lq, int n_seg, int seg_len, int hd,
                                         float scale, int q_prescaled, int kv_batches, float score_bound,
                                         void* workspace, int64_t workspace_bytes, void* stream) {
  AttnParams p;
  const int rc = mode_params(p, OSK_ATTN_BF16, nullptr, nullptr, 3, score_bound, q, q_batch_stride, q_row_stride, k, k_seg_stride,
                             k_batch_stride, k_row_stride, vt, vt_seg_stride, out, o_batch_stride, o_row_stride, lse, B, H, Lq, n_seg,
                             seg_len, hd, scale, q_prescaled, kv_batches, workspace, workspace_bytes);
  if (rc != OSK_OK) return rc;
  return dispatch(p, hd, OSK_ATTN_BF16, workspace, workspace_bytes, (hipStream_t)stream);
}

// ---- auto-dispatched pair (round 6): the bound comes from the operands themselves, per (batch, head), on the device
extern "C" int osk_attention_fwd_auto_bf16(const void* q, int64_t q_batch_stride, int64_t q_row_stride,
                                           const void* k, int64_t k_seg_stride, int64_t k_batch_stride,
                                           int64_t k_row_stride, const void* vt, int64_t vt_seg_stride,
                                           void* out, int64_t o_batch_stride, int64_t o_row_stride,
                                           float* lse, int B, int H, int Lq, int n_seg, int seg_len, int hd,
                                           float scale, int q_prescaled, int kv_batches, const float* q_norm2_max,
                                           const float* k_norm2_max, void* workspace, int64_t workspace_bytes, void* stream) {
  if (!q_norm2_max || !k_norm2_max || ((uintptr_t)q_norm2_max & 3) || ((uintptr_t)k_norm2_max & 3)) return OSK_EINVAL;
  AttnParams p;
  int rc = attn_params(p, q, q_batch_stride, q_row_stride, k, k_seg_stride, k_batch_stride, k_row_stride, vt, vt_seg_stride, 7,
                       out, o_batch_stride, o_row_stride, lse, B, H, Lq, n_seg, seg_len, hd, {64, 72, 128}, scale, q_prescaled,
                       kv_batches, workspace, workspace_bytes);
  if (rc != OSK_OK) return rc;
  if (!q_prescaled && scale * 1.4426950408889634f != 1.0f) return OSK_EUNSUPPORTED;   // the norms must be those of the operands the MFMA sees
  p.sc = 1.0f;
  p.q_prescaled = 1;
  hipStream_t st = (hipStream_t)stream;
  p.bound = 1.0f;                                  // "a bound exists": the FAST body's layout rules (attn_fast_path)
  if (!osk_attn::attn_fast_path(p)) {              // several key segments of fewer than 3 tiles: only the general body takes them
    p.bound = 0.f;
    launch_shape(p, hd, workspace, workspace_bytes);
    return then_merge(run(p, hd, st), p, hd, st);
  }
  // the FAST twin: launch shape as a bounded call's (wide layout, tail split), every workgroup checks its own (batch, head)
  p.qn2 = q_norm2_max; p.kn2 = k_norm2_max;
  launch_shape(p, hd, workspace, workspace_bytes);
  rc = run(p, hd, st);
  if (rc != 0) return rc;
  // the general twin: 256-row units, no tail split (its units write their final rows; the merge kernel skips them)
  AttnParams g = p;
  g.bound = 0.f; g.rows = 256; g.tail_split = 1; g.tail_first = 0x7fffffff; g.ws_o = nullptr; g.ws_lse = nullptr;
  return then_merge(run(g, hd, st), p, hd, st);
}

// squared row norms of a bf16 [B, L, H * hd] view, maximum per (batch, head): out[b * H + h] = max_l sum_d x[b, l, h, d]^2  (f32).
// HBM-bound: one read of the tensor.  accumulate != 0 keeps the values already in `out` (several key segments / sequence-parallel ranks
// fold into one maximum); else out is zeroed first (stream-ordered).  Non-negative floats order like their bit patterns: integer atomics.
namespace {
__global__ void zero_u32_kernel(unsigned* __restrict__ p, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) p[i] = 0u;
}

template <int HD>
__global__ void __launch_bounds__(256) rownorm2_max_kernel(const unsigned short* __restrict__ x, int64_t bs, int64_t rs, int L, int H,
                                                           int rows_per_block, unsigned* __restrict__ out) {
  __shared__ unsigned smax[256];
  const int b = blockIdx.y;
  for (int i = threadIdx.x; i < H; i += 256) smax[i] = 0;
  __syncthreads();
  const int r0 = blockIdx.x * rows_per_block;
  const int r1 = r0 + rows_per_block < L ? r0 + rows_per_block : L;
  const int pairs = (r1 - r0) * H;                       // (row, head) pairs of this block's slab, head fastest
  constexpr int CPR = HD / 8;
  for (int i = threadIdx.x; i < pairs; i += 256) {
    const int r = r0 + i / H, h = i - (i / H) * H;
    const unsigned short* px = x + b * bs + (int64_t)r * rs + h * HD;
    uint4 u[CPR];
#pragma unroll
    for (int c = 0; c < CPR; ++c) u[c] = *reinterpret_cast<const uint4*>(px + c * 8);   // all loads first
    float ss = 0.f;
#pragma unroll
    for (int c = 0; c < CPR; ++c) {
      float f[8];
      unpack8(u[c], f);
#pragma unroll
      for (int j = 0; j < 8; ++j) ss += f[j] * f[j];
    }
    atomicMax(&smax[h], __float_as_uint(ss));
  }
  __syncthreads();
  for (int i = threadIdx.x; i < H; i += 256)
    if (smax[i]) atomicMax(&out[b * H + i], smax[i]);
}
}  // namespace

extern "C" int osk_rownorm2_max_bf16(const void* x, int64_t batch_stride, int64_t row_stride, int B, int L, int H, int hd,
                                     float* out, int accumulate, void* stream) {
  if (!x || !out || B <= 0 || L <= 0 || H <= 0 || H > 256 || (batch_stride & 7) || (row_stride & 7) || ((uintptr_t)x & 15) || ((uintptr_t)out & 3))
    return OSK_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  // (zeroed by a KERNEL, not hipMemsetAsync: under hipGraph capture the memset of these few bytes was not replayed -- a replayed step
  //  then folded its maxima into the previous replay's, found by tests/test_gpu_mmdit.py::test_denoise_step_is_hipgraph_capturable[device_bound])
  if (!accumulate) hipLaunchKernelGGL(zero_u32_kernel, dim3((B * H + 255) / 256), dim3(256), 0, st, reinterpret_cast<unsigned*>(out), B * H);
  int rows = (L + 255) / 256;             // about 256 blocks per batch item: few, fat blocks (same-address atomics are slow)
  if (rows < 16) rows = 16;
  dim3 grid((L + rows - 1) / rows, B), block(256);
  unsigned* o = reinterpret_cast<unsigned*>(out);
  if (hd == 64) hipLaunchKernelGGL(rownorm2_max_kernel<64>, grid, block, 0, st, (const unsigned short*)x, batch_stride, row_stride, L, H, rows, o);
  else if (hd == 72) hipLaunchKernelGGL(rownorm2_max_kernel<72>, grid, block, 0, st, (const unsigned short*)x, batch_stride, row_stride, L, H, rows, o);
  else if (hd == 128) hipLaunchKernelGGL(rownorm2_max_kernel<128>, grid, block, 0, st, (const unsigned short*)x, batch_stride, row_stride, L, H, rows, o);
  else return OSK_EUNSUPPORTED;
  return (int)hipGetLastError();
}

extern "C" int osk_attention_fwd_ws_bf16(const void* q, int64_t q_batch_stride, int64_t q_row_stride,
                                         const void* k, int64_t k_seg_stride, int64_t k_batch_stride,
                                         int64_t k_row_stride, const void* vt, int64_t vt_seg_stride,
                                         void* out, int64_t o_batch_stride, int64_t o_row_stride,
                                         float* lse, int B, int H, int Lq, int n_seg, int seg_len, int hd,
                                         float scale, int q_prescaled, int kv_batches, void* workspace,
                                         int64_t workspace_bytes, void* stream) {
  return osk_attention_fwd_bounded_bf16(q, q_batch_stride, q_row_stride, k, k_seg_stride, k_batch_stride, k_row_stride, vt,
                                        vt_seg_stride, out, o_batch_stride, o_row_stride, lse, B, H, Lq, n_seg, seg_len, hd,
                                        scale, q_prescaled, kv_batches, 0.0f, workspace, workspace_bytes, stream);
}

extern "C" const char* osk_attention_kernel_name(int hd, int seg_len) {
  (void)seg_len;
  return hd == 72 ? "attn_asm72_kernel" : hd == 128 ? "attn_asm128_kernel" : hd == 64 ? "attn_asm72_kernel (head_dim 64 instantiation)" : "unsupported";
}

extern "C" const char* osk_attention_body_name(int hd, int n_seg, int seg_len, float score_bound) {
  if (hd != 64 && hd != 72 && hd != 128) return "unsupported";
  AttnParams p{};
  set_segments(p, n_seg, seg_len);
  if (score_bound > 0.f) p.bound = bound_to_bf16_up(score_bound);   // (negative / NaN: no bound, the general body)
  const bool fast = osk_attn::attn_fast_path(p);
  if (hd == 72 || hd == 64) return fast ? "attn_asm72_kernel<FAST>" : "attn_asm72_kernel<general>";   // (Lq >= 1024: the FAST body's wide layout, attn_asm72w_kernel)
  return fast ? "attn_asm128_kernel<FAST>" : "attn_asm128_kernel<general>";
}


// =============================================================================================
// fp8 P.V variant: V -> e4m3 V^T with the key order, ones row and zero rows the kernels expect; entry point
// =============================================================================================
namespace {

// V [B, L, H, hd] bf16 (strided) -> vt8 [B, H, RP, Lp] e4m3 bytes, RP = (hd + 1) rounded up to 16.
// One block = one 64-key tile of one head.  Row d < hd: byte hi*32 + t2*16 + j*4 + i of the tile holds key
// 32 t2 + 8 j + 4 hi + i (the order in which a lane of the score accumulators holds its 32 P values), quantised
// with the (batch, head) scale; row hd: 1.0 for keys < L, 0 behind them (softmax denominator / key validity);
// rows hd+1 .. RP-1: zero.
template <int HD>
__global__ void __launch_bounds__(256) v_transpose_fp8_kernel(const unsigned short* __restrict__ v, int64_t bs,
                                                              int64_t rs, const float* __restrict__ scales,
                                                              unsigned char* __restrict__ vt8, int L, int Lp, int H) {
  constexpr int RP = (HD + 1 + 15) / 16 * 16;
  __shared__ unsigned short tile[64][HD + 2];
  const int kt = blockIdx.x, h = blockIdx.y, b = blockIdx.z;
  const int key0 = kt * 64;
  constexpr int CPR = HD / 8;
  for (int i = threadIdx.x; i < 64 * CPR; i += 256) {
    const int r = i / CPR, c = i % CPR;
    const int key = key0 + r;
    uint4 u = make_uint4(0, 0, 0, 0);
    if (key < L) u = *reinterpret_cast<const uint4*>(v + b * bs + (int64_t)key * rs + h * HD + c * 8);
    unsigned* dst = reinterpret_cast<unsigned*>(&tile[r][c * 8]);
    dst[0] = u.x; dst[1] = u.y; dst[2] = u.z; dst[3] = u.w;
  }
  __syncthreads();
  // V / scale with an IEEE f32 division, as include/osk.h states and osk_k_pack_fp8 does: a product with the rounded reciprocal
  // moves a quotient that is an exact e4m3 tie (84.0 between 80 and 88) off the tie and rounds it away from the even neighbour
  const float scale = scales[b * H + h];
  unsigned char* obase = vt8 + ((int64_t)(b * H + h) * RP) * Lp + key0;
  // thread = (row, 16-byte chunk of the 64-byte row)
  for (int i = threadIdx.x; i < RP * 4; i += 256) {
    const int d = i >> 2, c = i & 3;
    unsigned w[4];
#pragma unroll
    for (int q4 = 0; q4 < 4; ++q4) {          // dword q4 of the chunk: bytes pos = c*16 + q4*4 + 0..3
      const int pos = c * 16 + q4 * 4;
      const int hi = pos >> 5, s5 = pos & 31, t2 = s5 >> 4, j = (s5 & 15) >> 2;
      const int k0 = 32 * t2 + 8 * j + 4 * hi;   // keys k0 .. k0 + 3
      if (d < HD) {
        float f[4];
#pragma unroll
        for (int e = 0; e < 4; ++e)
          f[e] = fminf(fmaxf(bf16_bits_to_f32(tile[k0 + e][d]) / scale, -448.0f), 448.0f);
        int r = 0;
        r = __builtin_amdgcn_cvt_pk_fp8_f32(f[0], f[1], r, false);
        r = __builtin_amdgcn_cvt_pk_fp8_f32(f[2], f[3], r, true);
        w[q4] = (unsigned)r;
      } else if (d == HD) {
        unsigned r = 0;
#pragma unroll
        for (int e = 0; e < 4; ++e) r |= (key0 + k0 + e < L ? 0x38u : 0u) << (8 * e);
        w[q4] = r;
      } else {
        w[q4] = 0;
      }
    }
    *reinterpret_cast<uint4*>(obase + (int64_t)d * Lp + c * 16) = make_uint4(w[0], w[1], w[2], w[3]);
  }
}

}  // namespace

namespace {

// absmax of V per (batch, head) -> e4m3 scale: bit patterns of |bf16| order like the values, so the reduction runs on
// integers.  grid (row slabs, B); a thread owns 16-byte chunks of the [H*hd] row (one head each), walks the slab's rows,
// then one LDS atomic per chunk and one global atomic per (block, head): few, fat blocks (same-address atomics are slow).
__global__ void __launch_bounds__(256) v_absmax_kernel(const unsigned short* __restrict__ v, int64_t bs, int64_t rs,
                                                       int L, int H, int hd, int rows_per_block,
                                                       unsigned* __restrict__ amax_bits) {
  __shared__ unsigned smax[256];
  const int b = blockIdx.y;
  for (int i = threadIdx.x; i < H; i += 256) smax[i] = 0;
  __syncthreads();
  const int cpr = (H * hd) >> 3;
  const int r0 = blockIdx.x * rows_per_block;
  const int r1 = r0 + rows_per_block < L ? r0 + rows_per_block : L;
  for (int c = threadIdx.x; c < cpr; c += 256) {
    const unsigned short* p = v + b * bs + c * 8;
    unsigned m = 0;
    int r = r0;
    for (; r + 3 < r1; r += 4) {
      uint4 u[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) u[i] = *reinterpret_cast<const uint4*>(p + (int64_t)(r + i) * rs);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const unsigned w[4] = {u[i].x, u[i].y, u[i].z, u[i].w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const unsigned a = w[j] & 0x7FFF7FFFu;
          m = max(m, max(a & 0xFFFFu, a >> 16));
        }
      }
    }
    for (; r < r1; ++r) {
      const uint4 u = *reinterpret_cast<const uint4*>(p + (int64_t)r * rs);
      const unsigned w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const unsigned a = w[j] & 0x7FFF7FFFu;
        m = max(m, max(a & 0xFFFFu, a >> 16));
      }
    }
    atomicMax(&smax[(c * 8) / hd], m);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < H; i += 256)
    if (smax[i]) atomicMax(&amax_bits[b * H + i], smax[i]);
}

__global__ void v_scale_finalize_kernel(unsigned* __restrict__ amax_bits, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float amax = __uint_as_float(amax_bits[i] << 16);
  reinterpret_cast<float*>(amax_bits)[i] = amax > 0.f ? amax / 448.0f : 1.0f;
}

}  // namespace

extern "C" int osk_v_scale_fp8(const void* v, int64_t bs, int64_t rs, float* scales, int B, int L, int H, int hd,
                               void* stream) {
  if (!v || !scales || B <= 0 || L <= 0 || H <= 0 || H > 256 || (hd & 7) || (bs & 7) || (rs & 7) || ((uintptr_t)v & 15))
    return OSK_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(zero_u32_kernel, dim3((B * H + 255) / 256), dim3(256), 0, st, reinterpret_cast<unsigned*>(scales), B * H);   // (a kernel, not hipMemsetAsync: see osk_rownorm2_max_bf16)
  int rows = (L + 127) / 128;            // about 128 blocks per batch item
  if (rows < 16) rows = 16;
  dim3 grid((L + rows - 1) / rows, B), block(256);
  hipLaunchKernelGGL(v_absmax_kernel, grid, block, 0, st, (const unsigned short*)v, bs, rs, L, H, hd, rows,
                     reinterpret_cast<unsigned*>(scales));
  hipLaunchKernelGGL(v_scale_finalize_kernel, dim3((B * H + 255) / 256), dim3(256), 0, st,
                     reinterpret_cast<unsigned*>(scales), B * H);
  return (int)hipGetLastError();
}

namespace {

// absmax of K AND of V per (batch, head) -> both e4m3 scale vectors from ONE launch: grid (H, B, 2), z = 0 K, z = 1 V.  A block
// owns one head of one batch item of one tensor over ALL L rows, so its maximum is final when it ends: no accumulator to zero,
// no cross-block atomic, no finalize pass (the three launches of osk_v_scale_fp8).  1024 threads = rpp rows x (hd / 8) 16-byte
// chunks of the head's columns per pass; the loads of U passes (U x 16 KB per workgroup at head_dim 128) are all issued before
// the first is folded.  Row indices past the end are clamped to L - 1: a repeated row does not move a maximum, and the tail
// needs no predicate.  Only 2 B H workgroups exist (48 for a rank of the 11B model at B = 1): a CU streamed 42 GB/s here with
// 8 and with 16 passes in flight alike, so below about 150 workgroups the CUs in use bound the launch, not HBM
// (profiles/attn_qk8_sp.md); splitting a head's rows over workgroups would need a zeroed accumulator, i.e. a second launch.
// The same integer maximum of |bf16| bit patterns and the same f32 division as v_absmax_kernel / v_scale_finalize_kernel.
constexpr int KV_SCALE_THREADS = 1024, KV_SCALE_U = 8;

__device__ __forceinline__ unsigned absmax_bits8(const uint4& u, unsigned m) {
  const unsigned w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const unsigned a = w[j] & 0x7FFF7FFFu;
    m = max(m, max(a & 0xFFFFu, a >> 16));
  }
  return m;
}

__global__ void __launch_bounds__(KV_SCALE_THREADS) kv_scale_fp8_kernel(const unsigned short* __restrict__ k, int64_t kbs, int64_t krs,
                                                                        const unsigned short* __restrict__ v, int64_t vbs, int64_t vrs,
                                                                        float* __restrict__ scales, int L, int H, int cpr, int rpp) {
  constexpr int U = KV_SCALE_U;
  __shared__ unsigned smax;
  const int h = blockIdx.x, b = blockIdx.y, z = blockIdx.z, B = gridDim.y;
  if (threadIdx.x == 0) smax = 0;
  __syncthreads();
  const int rl = threadIdx.x / cpr, c = threadIdx.x - rl * cpr;
  if (rl < rpp) {            // (hd / 8 does not divide 1024: the last few threads have no row)
    const unsigned short* p = (z ? v + b * vbs : k + b * kbs) + (int64_t)h * cpr * 8 + c * 8;
    const int64_t rs = z ? vrs : krs;
    unsigned m = 0;
    const int64_t last = L - 1;
    for (int64_t r = rl; r < L; r += (int64_t)U * rpp) {
      uint4 u[U];
#pragma unroll
      for (int i = 0; i < U; ++i) u[i] = *reinterpret_cast<const uint4*>(p + min(r + (int64_t)i * rpp, last) * rs);
#pragma unroll
      for (int i = 0; i < U; ++i) m = absmax_bits8(u[i], m);
    }
    if (m) atomicMax(&smax, m);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const float amax = __uint_as_float(smax << 16);
    scales[((int64_t)z * B + b) * H + h] = amax > 0.f ? amax / 448.0f : 1.0f;
  }
}

}  // namespace

extern "C" int osk_kv_scale_fp8(const void* k, int64_t kbs, int64_t krs, const void* v, int64_t vbs, int64_t vrs, float* scales,
                                int B, int L, int H, int hd, void* stream) {
  if (!k || !v || !scales || B <= 0 || B > 65535 || L <= 0 || H <= 0 || H > 256 || hd <= 0 || (hd & 7) || (kbs & 7) || (krs & 7) ||
      (vbs & 7) || (vrs & 7) || ((uintptr_t)k & 15) || ((uintptr_t)v & 15) || ((uintptr_t)scales & 3))
    return OSK_EINVAL;
  const int cpr = hd >> 3;
  if (cpr > KV_SCALE_THREADS) return OSK_EUNSUPPORTED;   // (a head row wider than one pass of the block: hd > 8192)
  hipLaunchKernelGGL(kv_scale_fp8_kernel, dim3(H, B, 2), dim3(KV_SCALE_THREADS), 0, (hipStream_t)stream, (const unsigned short*)k,
                     kbs, krs, (const unsigned short*)v, vbs, vrs, scales, L, H, cpr, KV_SCALE_THREADS / cpr);
  return (int)hipGetLastError();
}

extern "C" int osk_v_transpose_fp8(const void* v, int64_t bs, int64_t rs, const float* scales, void* vt8, int B, int L,
                                   int H, int hd, void* stream) {
  if (!v || !vt8 || !scales || B <= 0 || L <= 0 || H <= 0 || (bs & 7) || (rs & 7) || ((uintptr_t)vt8 & 15)) return OSK_EINVAL;
  const int Lp = (L + 63) / 64 * 64;
  dim3 grid(Lp / 64, H, B), block(256);
  hipStream_t st = (hipStream_t)stream;
  if (hd == 72)
    hipLaunchKernelGGL(v_transpose_fp8_kernel<72>, grid, block, 0, st, (const unsigned short*)v, bs, rs, scales, (unsigned char*)vt8, L, Lp, H);
  else if (hd == 128)
    hipLaunchKernelGGL(v_transpose_fp8_kernel<128>, grid, block, 0, st, (const unsigned short*)v, bs, rs, scales, (unsigned char*)vt8, L, Lp, H);
  else
    return OSK_EUNSUPPORTED;
  return (int)hipGetLastError();
}

extern "C" int osk_attention_fwd_pv8_bf16(const void* q, int64_t q_batch_stride, int64_t q_row_stride,
                                          const void* k, int64_t k_seg_stride, int64_t k_batch_stride,
                                          int64_t k_row_stride, const void* vt8, int64_t vt8_seg_stride,
                                          const float* v_scale, void* out, int64_t o_batch_stride, int64_t o_row_stride,
                                          float* lse, int B, int H, int Lq, int n_seg, int seg_len, int hd,
                                          float scale, int q_prescaled, int kv_batches, void* workspace,
                                          int64_t workspace_bytes, void* stream) {
  AttnParams p;
  const int rc = mode_params(p, OSK_ATTN_PV8, nullptr, v_scale, /* v_scale_mask: null is all this entry checks */ 0, 0.f, q, q_batch_stride,
                             q_row_stride, k, k_seg_stride, k_batch_stride, k_row_stride, vt8, vt8_seg_stride, out, o_batch_stride,
                             o_row_stride, lse, B, H, Lq, n_seg, seg_len, hd, scale, q_prescaled, kv_batches, workspace, workspace_bytes);
  if (rc != OSK_OK) return rc;
  return dispatch(p, hd, OSK_ATTN_PV8, workspace, workspace_bytes, (hipStream_t)stream);
}

// =============================================================================================
// fp8 QK^T variant (head_dim 128): K -> e4m3 in the layout the kernel's LDS-DMA copies; entry point
// =============================================================================================
namespace {

// K [B, L, H * 128] bf16 (strided) -> k8 [B, H, Lp, 128] e4m3 bytes, Lp = L rounded up to 64: byte d of row l = e4m3(clamp(k[b, l, h, d]
// / scales[b, h], +-448)), dims in their natural order; rows L .. Lp - 1 repeat row L - 1.  One block = one 64-key tile of one
// head; a thread converts 16-dim pieces (32 bytes in, 16 bytes out), all loads of a block in flight before the first use.
__global__ void __launch_bounds__(256) k_pack_fp8_kernel(const unsigned short* __restrict__ k, int64_t bs, int64_t rs,
                                                         const float* __restrict__ scales, unsigned char* __restrict__ k8, int L,
                                                         int Lp, int H) {
  const int kt = blockIdx.x, h = blockIdx.y, b = blockIdx.z;
  const float sc = scales[b * H + h];
  uint4 u[2][2];
  int row[2], c[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int j = threadIdx.x + 256 * i;       // 64 rows x 8 pieces
    row[i] = kt * 64 + (j >> 3);
    c[i] = j & 7;
    const int src = row[i] < L ? row[i] : L - 1;
    const unsigned short* px = k + b * bs + (int64_t)src * rs + h * 128 + c[i] * 16;
    u[i][0] = *reinterpret_cast<const uint4*>(px);
    u[i][1] = *reinterpret_cast<const uint4*>(px + 8);
  }
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    float f[16];
    unpack8(u[i][0], f);
    unpack8(u[i][1], f + 8);
    unsigned w[4];
#pragma unroll
    for (int q4 = 0; q4 < 4; ++q4) {
      float g[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) g[e] = fminf(fmaxf(f[q4 * 4 + e] / sc, -448.0f), 448.0f);
      int r = 0;
      r = __builtin_amdgcn_cvt_pk_fp8_f32(g[0], g[1], r, false);
      r = __builtin_amdgcn_cvt_pk_fp8_f32(g[2], g[3], r, true);
      w[q4] = (unsigned)r;
    }
    *reinterpret_cast<uint4*>(k8 + ((int64_t)(b * H + h) * Lp + row[i]) * 128 + c[i] * 16) = make_uint4(w[0], w[1], w[2], w[3]);
  }
}

}  // namespace

extern "C" int osk_k_pack_fp8(const void* k, int64_t bs, int64_t rs, const float* scales, void* k8, int B, int L, int H, int hd,
                              void* stream) {
  if (!k || !k8 || !scales || B <= 0 || L <= 0 || H <= 0 || (bs & 7) || (rs & 7) || ((uintptr_t)k & 15) || ((uintptr_t)k8 & 15) ||
      ((uintptr_t)scales & 3))
    return OSK_EINVAL;
  if (hd != 128) return OSK_EUNSUPPORTED;
  const int Lp = (L + 63) / 64 * 64;
  dim3 grid(Lp / 64, H, B), block(256);
  hipLaunchKernelGGL(k_pack_fp8_kernel, grid, block, 0, (hipStream_t)stream, (const unsigned short*)k, bs, rs, scales,
                     (unsigned char*)k8, L, Lp, H);
  return (int)hipGetLastError();
}

extern "C" int osk_attention_fwd_qk8_bf16(const void* q, int64_t q_batch_stride, int64_t q_row_stride,
                                          const void* k8, int64_t k8_seg_stride, int64_t k8_batch_stride,
                                          int64_t k8_row_stride, const float* k_scale, const void* vt8, int64_t vt8_seg_stride,
                                          const float* v_scale, void* out, int64_t o_batch_stride, int64_t o_row_stride,
                                          float* lse, int B, int H, int Lq, int n_seg, int seg_len, int hd,
                                          float scale, int q_prescaled, int kv_batches, void* workspace,
                                          int64_t workspace_bytes, void* stream) {
  AttnParams p;
  const int rc = mode_params(p, OSK_ATTN_QK8, k_scale, v_scale, 3, 0.f, q, q_batch_stride, q_row_stride, k8, k8_seg_stride, k8_batch_stride,
                             k8_row_stride, vt8, vt8_seg_stride, out, o_batch_stride, o_row_stride, lse, B, H, Lq, n_seg, seg_len, hd, scale,
                             q_prescaled, kv_batches, workspace, workspace_bytes);
  if (rc != OSK_OK) return rc;
  return dispatch(p, hd, OSK_ATTN_QK8, workspace, workspace_bytes, (hipStream_t)stream);
}

// =============================================================================================
// Ragged last key segment (sequence parallelism over a token count the rank count does not divide): two launches + one merge
// =============================================================================================
// The kernels bake ONE ragged-tile mask per launch (seg_len is uniform), so the n_seg - 1 full segments and the shorter last one
// are two launches of the normal selector; the second writes f32 partials (the split-tail epilogue, every unit, one part) that
// attn_merge_into_kernel folds into the first launch's rows in place.
static int64_t ragged_partial_bytes(int B, int H, int Lq, int hd) {
  return ((int64_t)((Lq + 255) / 256) * B * H * 256 * (hd + 1) * 4 + 15) & ~(int64_t)15;
}
static int64_t ragged_lse_bytes(int B, int H, int Lq) { return ((int64_t)B * H * Lq * 4 + 15) & ~(int64_t)15; }

extern "C" int64_t osk_attention_ragged_workspace_bytes(int B, int H, int Lq, int hd) {
  if (B <= 0 || H <= 0 || Lq <= 0 || hd <= 0) return 0;
  return ragged_partial_bytes(B, H, Lq, hd) + ragged_lse_bytes(B, H, Lq) + osk_attention_workspace_bytes();
}

// ---- the two-launch scheme the ragged entry and the window entries share: launch A writes finished rows, launch B -- over other keys --
// writes an f32 partial per unit, attn_merge_into_kernel folds B into A's rows in place.
// workspace: [f32 partials of launch B | lse of launch A when the caller keeps none | the rest: a tail split of launch A's own]
//
// What a call of the scheme must satisfy, checked with the entry's other OSK_EINVAL checks (in front of mode_params(), so that a malformed
// call is reported as malformed whatever head dim it asks for): the merge reads and writes `out` in 16-byte pieces, and the partials are
// not optional, so neither is the workspace.
static bool merge_args_ok(const void* out, int64_t o_batch_stride, int64_t o_row_stride, const float* lse, int B, int H, int Lq, int hd,
                          const void* workspace, int64_t workspace_bytes) {
  if (((uintptr_t)out & 15) || (o_batch_stride & 7) || (o_row_stride & 7) || !workspace) return false;
  return !(B > 0 && H > 0 && Lq > 0 && hd > 0 && workspace_bytes < ragged_partial_bytes(B, H, Lq, hd) + (lse ? 0 : ragged_lse_bytes(B, H, Lq)));
}

static float* borrowed_lse(void* workspace, int B, int H, int Lq, int hd) {
  return (float*)((char*)workspace + ragged_partial_bytes(B, H, Lq, hd));
}

// a parameter block -> the every-unit partial launch: 256-row units, each writes an f32 partial O + the log2-domain lse of its whole key range
static void partial_launch(AttnParams& p, int hd, void* workspace) {
  p.rows = 256;
  p.tail_first = 0; p.tail_split = 1;
  p.ws_o = (float*)workspace;
  p.ws_lse = p.ws_o + (int64_t)osk_attn::attn_units(p) * 256 * hd;
}

// launch A (finished rows; its lse borrowed from the workspace when the caller keeps none), launch B as the partial launch, the merge.
// dispatch_a: A goes through dispatch() with the rest of the workspace, else it is launched as the caller shaped it.
static int run_pair(AttnParams& a, AttnParams& b, int hd, int mode, bool dispatch_a, void* workspace, int64_t workspace_bytes, hipStream_t st) {
  const int64_t used = ragged_partial_bytes(a.B, a.H, a.Lq, hd) + (a.lse ? 0 : ragged_lse_bytes(a.B, a.H, a.Lq));
  if (!a.lse) a.lse = borrowed_lse(workspace, a.B, a.H, a.Lq, hd);
  partial_launch(b, hd, workspace);
  int rc = dispatch_a ? dispatch(a, hd, mode, workspace_bytes > used ? (char*)workspace + used : nullptr, workspace_bytes - used, st)
                      : run_mode(a, hd, mode, st);
  if (rc != 0) return rc;
  rc = run_mode(b, hd, mode, st);
  if (rc != 0) return rc;
  b.out = a.out; b.lse = a.lse;
  return osk_attn::launch_merge_into(b, hd, 0.6931471805599453f, st);
}

// The same with TWO partial launches over two further key sets (the anchored window entry: prefix B, suffix C) and ONE three-part merge.
// workspace: [f32 partials of launch B | f32 partials of launch C | lse of launch A when the caller keeps none].  Launch A is launched as
// the caller shaped it; B and C share the unit order (p.map) and the slot layout, which is all the merge needs of them.
static int run_triple(AttnParams& a, AttnParams& b, AttnParams& c, int hd, int mode, void* workspace, hipStream_t st) {
  const int64_t part = ragged_partial_bytes(a.B, a.H, a.Lq, hd);
  if (!a.lse) a.lse = (float*)((char*)workspace + 2 * part);
  partial_launch(b, hd, workspace);
  partial_launch(c, hd, (char*)workspace + part);
  int rc = run_mode(a, hd, mode, st);
  if (rc != 0) return rc;
  rc = run_mode(b, hd, mode, st);
  if (rc != 0) return rc;
  rc = run_mode(c, hd, mode, st);
  if (rc != 0) return rc;
  b.out = a.out; b.lse = a.lse;
  return osk_attn::launch_merge_into2(b, c.ws_o, c.ws_lse, hd, 0.6931471805599453f, st);
}

extern "C" int osk_attention_fwd_ragged_bf16(const void* q, int64_t q_batch_stride, int64_t q_row_stride,
                                             const void* k, int64_t k_seg_stride, int64_t k_batch_stride, int64_t k_row_stride,
                                             const float* k_scale, const void* vt, int64_t vt_seg_stride, const float* v_scale,
                                             void* out, int64_t o_batch_stride, int64_t o_row_stride, float* lse,
                                             int B, int H, int Lq, int n_seg, int seg_len, int last_seg_len, int hd,
                                             float scale, int q_prescaled, int kv_batches, float score_bound, int mode,
                                             void* workspace, int64_t workspace_bytes, void* stream) {
  if (n_seg < 2 || last_seg_len < 1 || last_seg_len > seg_len) return OSK_EINVAL;
  if (!merge_args_ok(out, o_batch_stride, o_row_stride, lse, B, H, Lq, hd, workspace, workspace_bytes)) return OSK_EINVAL;
  AttnParams a;
  const int rc = mode_params(a, mode, k_scale, v_scale, 3, score_bound, q, q_batch_stride, q_row_stride, k, k_seg_stride, k_batch_stride,
                             k_row_stride, vt, vt_seg_stride, out, o_batch_stride, o_row_stride, lse, B, H, Lq, n_seg - 1, seg_len, hd, scale,
                             q_prescaled, kv_batches, workspace, workspace_bytes);
  if (rc != OSK_OK) return rc;
  // launch B: the last segment alone, laid out as a tensor of last_seg_len keys of its own (V^T rows of round_up(last_seg_len, 64)
  // positions; e4m3 K [Bkv, H, that many rows, 128], hence a batch stride of its own) n_seg - 1 segment strides in; same queries,
  // scales, bound
  AttnParams b = a;
  if (!lse) b.lse = borrowed_lse(workspace, B, H, Lq, hd);   // (as launch A; a partial launch writes none)
  set_segments(b, 1, last_seg_len);
  const int64_t skip = n_seg - 1;
  if (b.k) b.k += skip * a.kss;
  if (b.k8) { b.k8 += skip * a.kss; b.kbs = (int64_t)H * b.seg_lp * 128; }
  if (b.vt) b.vt += skip * a.vtss;
  if (b.vt8) b.vt8 += skip * a.vtss;
  // launch A through dispatch(): the launch shape of a plain call over the full segments (wide layout, tail split from the rest of the workspace)
  return run_pair(a, b, hd, mode, /* dispatch_a */ true, workspace, workspace_bytes, (hipStream_t)stream);
}

// =============================================================================================
// Per query block key windows with an always-attended key prefix (frame-window attention): two launches + one merge
// =============================================================================================
// Keys [0, n_prefix) (text) are seen by every query; keys [n_prefix, Lk) are the body, of which 256-row query block qb sees the
// 64-key tiles [first, first + count) of its table row and nothing else.  Launch A runs over the body as a key axis of its own
// -- K and V^T advanced by n_prefix keys, V^T's row stride still that of the whole tensor -- with the table (key_part() hands
// every work unit its run of tiles) and writes finished rows; launch B runs over the prefix as the partial launch of run_pair()
// (tail_first = 0, tail_split = 1) and attn_merge_into_kernel folds it into launch A's rows in place.
extern "C" int64_t osk_attention_window_workspace_bytes(int B, int H, int Lq, int hd) {
  if (B <= 0 || H <= 0 || Lq <= 0 || hd <= 0) return 0;
  return ragged_partial_bytes(B, H, Lq, hd) + ragged_lse_bytes(B, H, Lq);
}
// anchored (osk_attention_fwd_window_anchor_bf16): two partial sets -- the prefix launch's and the suffix launch's -- and launch A's lse
extern "C" int64_t osk_attention_window_anchor_workspace_bytes(int B, int H, int Lq, int hd) {
  if (B <= 0 || H <= 0 || Lq <= 0 || hd <= 0) return 0;
  return 2 * ragged_partial_bytes(B, H, Lq, hd) + ragged_lse_bytes(B, H, Lq);
}

// One function behind osk_attention_fwd_window_bf16 (mode OSK_ATTN_BF16, score_bound) and osk_attention_fwd_window_fp8_bf16 (the fp8
// operands of osk_attention_fwd_pv8_bf16 -- OSK_ATTN_PV8: bf16 K in place, e4m3 V^T -- or of osk_attention_fwd_qk8_bf16 -- OSK_ATTN_QK8:
// e4m3 K too, head_dim 128), driven through the kernels of the mode the way the ragged entry drives them.  What the loops meet is nothing
// the single-segment tail split does not already hand them: key_part()'s `win` branch gives the loaders a run of tiles (offsets of its
// first tile, tps = nt = its length, ragged only where it ends in the last tile); the fp8 kernels bake key validity into V^T's row hd (no
// first-tile LDS mask to write), their slot words see only `ragged`, and the q8 K loader steps whole 64 x 128-byte tiles from k_off = first
// tile * 64 * krs with krs = 128 (tests/attention_cases.py: p72_1tile_ragged, p72_merge, q128_1tile_ragged_plain, q128_tile_runs_merge run
// 1- and 2-tile parts, full and ragged).
// Launch A does not go through dispatch(): it keeps rows = 256, tail_first = 0x7fffffff, tail_split = 1 (the table is per 256 rows and a
// windowed unit has a key run of its own; split_tail() would return at p.win anyway, and only launch_shape() -- bf16 mode -- ever picks
// the wide layout).
// n_suffix > 0 (osk_attention_fwd_window_anchor_bf16): the last n_suffix keys [s0, Lk), s0 = Lk - n_suffix a multiple of 64 beyond n_prefix,
// are always attended as well.  The body -- and the table's tile axis -- then ends at s0 (whole tiles: launch A is never ragged), and
// launch C walks the suffix for every query as a partial launch entered s0 keys in, exactly as launch A enters n_prefix keys in: the ragged
// last tile of the tensor is the ragged last tile of a launch over n_suffix keys.  B and C fold into A's rows in ONE pass (run_triple());
// without a prefix C alone does, through run_pair().  n_suffix == 0 is the code path from before, launch for launch.
static int window_fwd(int mode, const void* q, int64_t q_batch_stride, int64_t q_row_stride, const void* k, int64_t k_batch_stride,
                      int64_t k_row_stride, const float* k_scale, const void* vt, const float* v_scale, void* out, int64_t o_batch_stride,
                      int64_t o_row_stride, float* lse, int B, int H, int Lq, int Lk, int n_prefix, int hd, float scale, int q_prescaled,
                      int kv_batches, float score_bound, const int32_t* windows, int n_windows, void* workspace, int64_t workspace_bytes,
                      void* stream, int n_suffix = 0) {
  if (!windows || ((uintptr_t)windows & 3)) return OSK_EINVAL;
  if (Lq <= 0 || Lk <= 0 || n_windows != (Lq + 255) / 256 || n_prefix < 0 || (n_prefix & 63) || n_prefix >= Lk) return OSK_EINVAL;
  // the suffix starts on a tile of the whole tensor and leaves the body at least one tile (s0 <= n_prefix: a suffix that reaches the prefix)
  if (n_suffix < 0 || (n_suffix > 0 && (((Lk - n_suffix) & 63) || Lk - n_suffix <= n_prefix))) return OSK_EINVAL;
  const int s0 = Lk - n_suffix;
  // (n_prefix == 0 and n_suffix == 0: a single launch, no partials, no workspace)
  if ((n_prefix > 0 || n_suffix > 0) && !merge_args_ok(out, o_batch_stride, o_row_stride, lse, B, H, Lq, hd, workspace, workspace_bytes))
    return OSK_EINVAL;
  if (n_prefix > 0 && n_suffix > 0 && B > 0 && H > 0 && hd > 0 &&
      workspace_bytes < 2 * ragged_partial_bytes(B, H, Lq, hd) + (lse ? 0 : ragged_lse_bytes(B, H, Lq)))
    return OSK_EINVAL;
  AttnParams a;
  const int rc = mode_params(a, mode, k_scale, v_scale, 3, score_bound, q, q_batch_stride, q_row_stride, k, 0, k_batch_stride, k_row_stride, vt,
                             0, out, o_batch_stride, o_row_stride, lse, B, H, Lq, 1, Lk, hd, scale, q_prescaled, kv_batches, workspace,
                             workspace_bytes);
  if (rc != OSK_OK) return rc;
  a.rows = 256;                                  // the table is per 256-row block; tail_first stays off: finished rows
  // Both launches walk a key range of ONE tensor laid out for all Lk keys: V^T [Bkv, H, hd | RP, Lp] and, in qk8 mode, K [Bkv, H, Lp, 128]
  // with Lp = round_up(Lk, 64).  The kernels take a head's stride from seg_lp (rows * seg_lp positions of V^T, seg_lp * 128 bytes of e4m3
  // K) and a V^T row's from seg_lp as well, so seg_lp stays the whole tensor's after set_segments() below.  kbs needs no such care here: it
  // is the caller's batch stride of that one tensor (H * Lp * 128 when packed), which set_segments() does not touch -- the ragged entry
  // re-derives it only because its last segment is a tensor of its own with another Lp.
  const int64_t seg_lp = a.seg_lp;
  AttnParams b = a, c = a;
  // launch A: the body, windowed, entered n_prefix keys in.  bf16 K: n_prefix rows of krs elements.  e4m3 K: n_prefix rows of 128
  // bytes inside every head's [Lp, 128] block.  V^T: n_prefix positions along the key axis of EVERY row -- in the e4m3 layout the hd dims
  // and the validity / denominator row hd alike, since all rows of a head share the one base pointer and the row stride seg_lp.  n_prefix
  // is a multiple of 64, so the body's tiles are tiles of the whole tensor: the key order inside a tile, the repeated last K row and the
  // zero validity bytes behind key Lk - 1 sit where a launch over Lk - n_prefix keys expects its ragged last tile.
  if (a.k) a.k += (int64_t)n_prefix * a.krs;
  if (a.k8) a.k8 += (int64_t)n_prefix * 128;
  if (a.vt) a.vt += n_prefix;
  if (a.vt8) a.vt8 += n_prefix;
  set_segments(a, 1, s0 - n_prefix);
  a.seg_lp = (int)seg_lp;
  a.win = windows;
  if (n_prefix == 0 && n_suffix == 0) return run_mode(a, hd, mode, (hipStream_t)stream);
  // launch B: the prefix alone from the tensors' origin -- whole tiles (n_prefix % 64 == 0: never ragged), the same scales and bound
  set_segments(b, 1, n_prefix);
  b.seg_lp = (int)seg_lp;
  if (n_suffix == 0) return run_pair(a, b, hd, mode, /* dispatch_a */ false, workspace, workspace_bytes, (hipStream_t)stream);
  // launch C: the suffix alone, entered s0 keys in by the rule of launch A; its last tile is the tensor's (ragged where Lk % 64 != 0)
  if (c.k) c.k += (int64_t)s0 * c.krs;
  if (c.k8) c.k8 += (int64_t)s0 * 128;
  if (c.vt) c.vt += s0;
  if (c.vt8) c.vt8 += s0;
  set_segments(c, 1, n_suffix);
  c.seg_lp = (int)seg_lp;
  if (n_prefix == 0) return run_pair(a, c, hd, mode, /* dispatch_a */ false, workspace, workspace_bytes, (hipStream_t)stream);
  return run_triple(a, b, c, hd, mode, workspace, (hipStream_t)stream);
}

extern "C" int osk_attention_fwd_window_bf16(const void* q, int64_t q_batch_stride, int64_t q_row_stride,
                                             const void* k, int64_t k_batch_stride, int64_t k_row_stride, const void* vt,
                                             void* out, int64_t o_batch_stride, int64_t o_row_stride, float* lse,
                                             int B, int H, int Lq, int Lk, int n_prefix, int hd, float scale, int q_prescaled,
                                             int kv_batches, float score_bound, const int32_t* windows, int n_windows,
                                             void* workspace, int64_t workspace_bytes, void* stream) {
  return window_fwd(OSK_ATTN_BF16, q, q_batch_stride, q_row_stride, k, k_batch_stride, k_row_stride, nullptr, vt, nullptr, out, o_batch_stride,
                    o_row_stride, lse, B, H, Lq, Lk, n_prefix, hd, scale, q_prescaled, kv_batches, score_bound, windows, n_windows, workspace,
                    workspace_bytes, stream);
}

extern "C" int osk_attention_fwd_window_fp8_bf16(const void* q, int64_t q_batch_stride, int64_t q_row_stride,
                                                 const void* k, int64_t k_batch_stride, int64_t k_row_stride, const float* k_scale,
                                                 const void* vt, const float* v_scale, void* out, int64_t o_batch_stride,
                                                 int64_t o_row_stride, float* lse, int B, int H, int Lq, int Lk, int n_prefix, int hd,
                                                 float scale, int q_prescaled, int kv_batches, int mode, const int32_t* windows,
                                                 int n_windows, void* workspace, int64_t workspace_bytes, void* stream) {
  if (mode != OSK_ATTN_PV8 && mode != OSK_ATTN_QK8) return OSK_EINVAL;   // (OSK_ATTN_BF16: osk_attention_fwd_window_bf16)
  return window_fwd(mode, q, q_batch_stride, q_row_stride, k, k_batch_stride, k_row_stride, k_scale, vt, v_scale, out, o_batch_stride,
                    o_row_stride, lse, B, H, Lq, Lk, n_prefix, hd, scale, q_prescaled, kv_batches, 0.f, windows, n_windows, workspace,
                    workspace_bytes, stream);
}

// The window entries with always-attended trailing keys as well (anchor frames: MMDiTModel.set_attention_window(anchors=...)); one entry
// for the three operand kinds, as the ragged entry has.
extern "C" int osk_attention_fwd_window_anchor_bf16(const void* q, int64_t q_batch_stride, int64_t q_row_stride,
                                                    const void* k, int64_t k_batch_stride, int64_t k_row_stride, const float* k_scale,
                                                    const void* vt, const float* v_scale, void* out, int64_t o_batch_stride,
                                                    int64_t o_row_stride, float* lse, int B, int H, int Lq, int Lk, int n_prefix,
                                                    int n_suffix, int hd, float scale, int q_prescaled, int kv_batches, float score_bound,
                                                    int mode, const int32_t* windows, int n_windows, void* workspace,
                                                    int64_t workspace_bytes, void* stream) {
  if (mode != OSK_ATTN_BF16 && mode != OSK_ATTN_PV8 && mode != OSK_ATTN_QK8) return OSK_EINVAL;
  return window_fwd(mode, q, q_batch_stride, q_row_stride, k, k_batch_stride, k_row_stride, k_scale, vt, v_scale, out, o_batch_stride,
                    o_row_stride, lse, B, H, Lq, Lk, n_prefix, hd, scale, q_prescaled, kv_batches, mode == OSK_ATTN_BF16 ? score_bound : 0.f,
                    windows, n_windows, workspace, workspace_bytes, stream, n_suffix);
}
