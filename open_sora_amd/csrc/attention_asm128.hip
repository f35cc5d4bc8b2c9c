// Flash-attention forward for head_dim 128 (the 11B MMDiT geometry), gfx950: hand-scheduled main loop.
//
// Same dataflow and generator as attention_asm72.hip (see tools/gen_attn_asm.py), 4 waves x 64 query rows, one wave
// per SIMD; what differs with 128 real dims:
//  * K tile = two swizzled 64-dim LDS images (dims 0..63, 64..127), 16 LDS-DMA instructions, 4 per wave;
//  * the reference max M rides in a NINTH, pure-padding QK^T k-step whose K fragment is a constant register quad
//    {1.0, 0, ...} (no LDS read) and whose Q fragment holds -M in dim 128;
//  * V^T tile = 128 dim rows + the ones row 128 (softmax denominator = accumulator row 128, a fifth O^T row tile).
// Numerics are those of the head_dim-72 kernel: P = exp2(S') with S' = q.k - M straight out of the MFMA, M moves only
// when a row max exceeds it by more than 8 (log2 units).
#include "attention_asm_wrap.h"
#include "attention_asm_regs.inc"

namespace osk_attn {
namespace {

constexpr int HD = 128, NKS = OSK128_NKS, NDT = OSK128_NDT, NU = 2, NW = 4, ROWS = 256, NSLOT = OSK128N2_NSLOT;
static_assert(NKS == 9 && NDT == 5 && NSLOT == 4, "generated geometry changed: update the wrapper");

template <bool FAST>   // FAST: a score bound was given (attention_params.h::attn_fast_path); any key count, any segment layout
__global__ void __launch_bounds__(256, 1) attn_asm128_kernel(const AttnParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const Work w = decode_work<ROWS>(p);
  const int lane = w.lane, wave = w.wave;
  float bound;   // the caller's score bound, or -- auto-dispatched pairs -- the one this (batch, head)'s operands imply (attention_params.h)
  if (!attn_auto_bound(p, w.b, w.h, FAST, bound)) return;
  (void)bound;   // (this head_dim's FAST body exponentiates the raw scores: the bound only decides which body runs)

  // ---- LDS: zero (rows 129..159 of the V^T slots stay zero for good), ones row 128 of both V^T slots
  clear_lds<OSK128_SMEM, NW>(smem, w.tid);
  __syncthreads();
  lds_ones_rows<OSK128_VOFF0, OSK128_VTILE, HD>(smem, w.tid);
  // ragged last key tile of a segment: see attention_asm72.hip (clamped K rows + validity-mask ones row)
  const int last_valid = p.seg_len - (p.tps - 1) * 64;
  const KeyPart kp = key_part(p, w.tail, w.part, w.qb, last_valid < 64);   // the whole key axis, or one part of a split tail unit
  const bool ragged = kp.ragged;
  unsigned maskval = 0;
  if (lane < 32) {
    // row 128 is not swizzled ((128 >> 1) & 7 == 0): dword `lane` = columns 2 lane, 2 lane + 1 of the V^T tile,
    // whose baked key order is key = 16 (c / 16) + perm(c % 16)
    const int c0 = lane * 2, c1 = c0 + 1;
    auto key_of = [](int c) { const int j = c & 15; return (c & ~15) + ((j & 3) | ((j & 4) << 1) | ((j & 8) >> 1)); };
    maskval = (key_of(c0) < last_valid ? 0x3F80u : 0u) | (key_of(c1) < last_valid ? 0x3F800000u : 0u);
  }
  lds_mask_first_tile<OSK128_VOFF0, HD>(smem, w.tid, kp, maskval);
  __syncthreads();

  // ---- Q fragments; k-step 8 = padding (zero; dim 128 receives -M in the asm)
  // FAST: with a score bound B <= 56 no softmax reference is needed for range control: the body skips the padding k-step
  // (whose only job is to carry the reference through the MFMA) and exponentiates the raw scores, P = exp2(s) in
  // [2^-56, 2^56]; O and the row sum carry the same factor (attention_asm128_n2_f0.inc, tools/gen_attn_asm.py "nom")
  int qi[NU];
  osk_v4f qv[NU * NKS];
  load_q_bf16<HD, HD, NKS, NU, ROWS>(p, w, qi, qv);

  unsigned koff[NSLOT], koffL[NSLOT], voff[NSLOT];
  k_offsets128<NW, NSLOT>(p, w, last_valid, koff, koffL);
  vt_offsets<HD, NW, NSLOT>(p, w, voff);
  const unsigned lds_base = lds_address(smem);
  unsigned fo[4];
  k_frag_addrs(w, lds_base, fo);
  const unsigned onesaddr = lds_base + OSK128_VOFF0 + HD * 128 + lane * 4;   // lanes 32..63: the zero row behind it

  const int bkv = w.b % p.Bkv;
  const KLoader kl = k_loader<HD>(p, w, kp, bkv, lds_base);
  const VLoader vl = vt_loader<HD, OSK128_VOFF0, NW>(p, w, kp, p.vt, bkv, lds_base);
  const unsigned tps = rfl((unsigned)kp.tps), nt = rfl((unsigned)kp.nt);
  const unsigned nvw = rfl((unsigned)NSLOT | (ragged ? 0u : 1u << 8) | ((ragged && wave == 0) ? 1u << 9 : 0u));

  float m_ref[2];
#define OSK128_OPERANDS                                                                                               \
  : "=&v"(m_ref[0]), "=&v"(m_ref[1])                                                                                  \
  : "v"(koff[0]), "v"(koff[1]), "v"(koff[2]), "v"(koff[3]), "v"(voff[0]), "v"(voff[1]), "v"(voff[2]), "v"(voff[3]),   \
    "v"(fo[0]), "v"(fo[1]), "v"(fo[2]), "v"(fo[3]), "v"(koffL[0]), "v"(koffL[1]), "v"(koffL[2]), "v"(koffL[3]),       \
    "v"(maskval), "v"(onesaddr), "s"(kl.base), "s"(vl.base),                                                          \
    "s"(kl.step), "s"(kl.jump), "s"(vl.jump), "s"(tps), "s"(nt), "s"(kl.dst), "s"(vl.dst), "s"(nvw),                  \
    OSK_AQ_IN_40_5(qv), OSK_AQ_IN_45_4(qv + 5), OSK_AQ_IN_49_5(qv + 9), OSK_AQ_IN_54_4(qv + 14)
  if constexpr (FAST) {
    asm volatile(
#include "attention_asm128_n2_f0.inc"
        OSK128_OPERANDS : OSK128N2_CLOBBERS);
    m_ref[0] = m_ref[1] = 0.f;   // reference point of the exponentials: 0
  } else {
    asm volatile(
#include "attention_asm128_n2_v0.inc"
        OSK128_OPERANDS : OSK128N2_CLOBBERS);
  }

  // the O^T accumulators as values the compiler knows (acc_quads.h): outputs of an empty statement right behind the loop
  static_assert(OSK128N2_AQ0 == 160 && OSK128N2_AQ1 == 196 && OSK128N2_AO_REGS == 160,
                "the generated loops' register map: the operand lists above and below bind exactly these AGPRs");
  osk_v4f ov[40];
  asm volatile("" : OSK_AQ_OUT_0_40(ov));
  // row 128 of O^T = sum_k P: row 0 of row tile 4 = lanes hi == 0, register 0
  store_row_tiles<HD, NDT, NU, 4, 0, ROWS>(ov, 1.0f, m_ref, p, w, qi);
}

}  // namespace

int launch_asm128(const AttnParams& p, hipStream_t st) {
  return attn_fast_path(p) ? launch_kernel<attn_asm128_kernel<true>>(OSK128_SMEM, p, st) : launch_kernel<attn_asm128_kernel<false>>(OSK128_SMEM, p, st);
}

}  // namespace osk_attn
