// Flash-attention forward for head_dim 72 (DiT-XL geometry), gfx950: hand-scheduled main loop.
//
// Structure: 4 waves x 64 query rows, one wave per SIMD (the generator can also emit 8 waves x 32 rows, two per SIMD),
// LDS-DMA staged 64-key tiles, swapped operands: S^T = K . Q^T on v_mfma_f32_32x32x16_bf16 (80 padded dims), O^T += V^T . P^T
// on v_mfma_f32_16x16x32_bf16 (80 padded rows = 5 blocks of 16 instead of 3 x 32; P crosses from the 32-query score layout
// to the 16-query operand layout by one v_permlane16_swap per packed register pair), and the whole K/V loop is ONE asm
// statement emitted by tools/gen_attn_asm.py (attention_asm72_n{NU}_v{VAR}.inc): explicit register file (O^T and Q in AGPRs, two score tiles,
// P and two 4-slot fragment rings in VGPRs), every MFMA shadow filled by hand with ~5 issue slots of LDS reads /
// exp2 / pack / max work, counted lgkmcnt waits, one barrier per tile.  See the generator's header for the
// dataflow; this file is the wrapper: LDS init, Q pre-scale, the asm operands, the epilogue.
//
// Numerics vs the compiler-scheduled attention_fwd.hip (head_dim 64; rounds 1-2 also had a head_dim-72 twin, attention_w64.hip):
//  * Q carries scale*log2(e): folded into q's single rounding by osk_qknorm_rope_bf16 (q_prescaled, the model path),
//    or applied here with one extra bf16 rounding of q (stand-alone calls);
//  * the online-softmax reference max M is kept bf16-exact inside the contraction (Q padding dim 72 = -M, K
//    padding dim 72 = 1.0), so P = exp2(S') with S' straight out of the MFMA; M moves only when a row max exceeds
//    it by more than 8 (log2 units): P <= 2^8, O and the row sum (ones row of V^T) carry the same factor.
// Any key count: a ragged last tile of a key segment re-fetches the segment's last key for the missing rows and masks
// them out of the denominator through the ones row (see the wrapper).
#include "attention_asm_wrap.h"
#include "attention_asm_regs.inc"

namespace osk_attn {
namespace {

constexpr int HDL = 72, NKS = 5;   // HDL: the head_dim of the LDS images / register layout; the tensors' head_dim is the template parameter HD (72, or 64: see below)

// HD = 64 (round 4: the S-width models; the compiler-scheduled attn_fwd_kernel<64> is gone): the SAME loop on tensors with 64-wide heads --
// Q's dims 64..71 are zero, K's 8-dim column image is never fetched (its LDS chunk stays zero: the loader slot that fetches it does not
// exist), V^T has 64 rows (LDS rows 64..71 stay zero), the ones row stays LDS row 72.  80 padded dims for 64 real ones: issued / useful 1.25.
template <bool FAST, int HD>   // FAST: a score bound was given (attention_params.h::attn_fast_path); any key count, any segment layout
__global__ void __launch_bounds__(256, 1) attn_asm72_kernel(const AttnParams p) {
  constexpr int ROWS = 256;                                    // query rows per workgroup
  constexpr int NU = 2;                                        // 32-row query blocks per wave (the generator's 8 waves x 32
  constexpr int NW = 8 / NU;                                   // rows layout tied this one in rounds 1-2 and is not shipped)
  constexpr int NSLOT = OSK72N2_NSLOT;                         // LDS-DMA slots per wave and tile
  static_assert(NSLOT == 3 && OSK72_NDB == 5, "generated geometry changed: update the wrapper");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const Work w = decode_work<ROWS>(p);
  const int lane = w.lane, wave = w.wave, hi = w.hi;
  float bound;   // the caller's score bound, or -- auto-dispatched pairs -- the one this (batch, head)'s operands imply (attention_params.h)
  if (!attn_auto_bound(p, w.b, w.h, FAST, bound)) return;

  // ---- LDS: zero, ones row of both V^T slots, constant chunk {1.0, 0 x 7} = K's padding dims 72..79
  clear_lds<OSK72_SMEM, NW>(smem, w.tid);
  __syncthreads();
  lds_ones_rows<OSK72_VOFF0, OSK72_VTILE, HDL>(smem, w.tid);
  lds_const_chunk<OSK72_CONST_OFF, OSK72_KTILE>(smem, w.tid);
  // ragged last key tile of a segment (seg_len % 64 != 0): K rows past the segment re-fetch its last key (finite
  // scores), V^T is zero there (osk_v_transpose_bf16 pads), and the tile's ones row becomes a validity mask so the
  // duplicates do not count in the softmax denominator.  The mask is in the V^T tile's baked key order.
  const int last_valid = p.seg_len - (p.tps - 1) * 64;   // keys in the last tile of a segment (1..64)
  const KeyPart kp = key_part(p, w.tail, w.part, w.qb, last_valid < 64);   // the whole key axis, or one part of a split tail unit
  const bool ragged = kp.ragged;
  const unsigned maskval = ragged_mask72(lane, last_valid);
  lds_mask_first_tile<OSK72_VOFF0, HDL>(smem, w.tid, kp, maskval);
  __syncthreads();

  int qi[NU];
  osk_v4f qv[NU * NKS];
  load_q_bf16<HD, HDL, NKS, NU, ROWS>(p, w, qi, qv);
  // FAST: the reference "max" is the caller's bound B, constant for the whole launch: Q's padding dim 72 (k-step 4, lanes
  // 32..63, word 0 low half) = -B against the 1.0 in K's padding dim -> the MFMA returns s - B directly, from tile 0 on
  if constexpr (FAST) {
#pragma unroll
    for (int u = 0; u < NU; ++u)
      if (hi) qv[u * NKS + 4][0] = __uint_as_float((__float_as_uint(-bound) >> 16) & 0xFFFFu);
  }

  unsigned koff[NSLOT], koffL[NSLOT], voff[NSLOT];
  k_offsets72<NW, NSLOT>(p, w, last_valid, koff, koffL);
  vt_offsets<HD, NW, NSLOT>(p, w, voff);
  const unsigned lds_base = lds_address(smem);
  unsigned fo[4], kc[2];
  k_frag_addrs(w, lds_base, fo);
  k_col_addrs72<OSK72_CONST_OFF>(w, lds_base, kc);
  const unsigned onesaddr = lds_base + OSK72_VOFF0 + HDL * 128 + lane * 4;   // lanes 32..63: the zero row behind it
  unsigned vo[2];
  vt_frag_addrs72(w, lds_base, vo);

  const int bkv = w.b % p.Bkv;   // key / value batch of this query batch
  const KLoader kl = k_loader<HD>(p, w, kp, bkv, lds_base);
  const VLoader vl = vt_loader<HD, OSK72_VOFF0, NW>(p, w, kp, p.vt, bkv, lds_base);
  const unsigned tpsnt = rfl((unsigned)kp.tps | ((unsigned)kp.nt << 16));   // (two operand slots went to vo[])
  const unsigned nkvw = loader_slots72<HD, NW, NSLOT>(wave, ragged);

  float m_ref[2];
#define OSK72_OPERANDS                                                                                                \
  : "=&v"(m_ref[0]), "=&v"(m_ref[1])                                                                                  \
  : "v"(koff[0]), "v"(koff[1]), "v"(koff[2]), "v"(voff[0]), "v"(voff[1]), "v"(voff[2]), "v"(fo[0]), "v"(fo[1]),       \
    "v"(fo[2]), "v"(fo[3]), "v"(kc[0]), "v"(kc[1]), "v"(koffL[0]), "v"(koffL[1]), "v"(koffL[2]), "v"(maskval),        \
    "v"(onesaddr), "v"(vo[0]), "v"(vo[1]), "s"(kl.base), "s"(vl.base),                                                \
    "s"(kl.step), "s"(kl.jump), "s"(vl.jump), "s"(tpsnt), "s"(kl.dst), "s"(vl.dst), "s"(nkvw),                        \
    OSK_AQ_IN_20_5(qv), OSK_AQ_IN_25_5(qv + 5)
  if constexpr (FAST) {
    asm volatile(
#include "attention_asm72_n2_f0.inc"
        OSK72_OPERANDS : OSK72N2_CLOBBERS);
    m_ref[0] = m_ref[1] = bound;
  } else {
    asm volatile(
#include "attention_asm72_n2_v0.inc"
        OSK72_OPERANDS : OSK72N2_CLOBBERS);
  }

  // the O^T accumulators as values the compiler knows (acc_quads.h): outputs of an empty statement right behind the loop
  static_assert(OSK72N2_AQ0 == 80 && OSK72N2_AQ1 == 100 && OSK72N2_AO_REGS == 80,
                "the generated loops' register map: the operand lists above and below bind exactly these AGPRs");
  osk_v4f ov[20];
  asm volatile("" : OSK_AQ_OUT_0_20(ov));

  store_row_blocks16<HD, NU, ROWS, true>(ov, m_ref, p, w);
}

}  // namespace

int launch_asm72(const AttnParams& p, hipStream_t st) {
  return attn_fast_path(p) ? launch_kernel<attn_asm72_kernel<true, 72>>(OSK72_SMEM, p, st) : launch_kernel<attn_asm72_kernel<false, 72>>(OSK72_SMEM, p, st);
}
int launch_asm64(const AttnParams& p, hipStream_t st) {
  return attn_fast_path(p) ? launch_kernel<attn_asm72_kernel<true, 64>>(OSK72_SMEM, p, st) : launch_kernel<attn_asm72_kernel<false, 64>>(OSK72_SMEM, p, st);
}

}  // namespace osk_attn
