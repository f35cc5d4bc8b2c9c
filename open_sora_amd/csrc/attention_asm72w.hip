// Flash-attention forward for head_dim 72, gfx950: the WIDE layout of the bounded (FAST) body -- round 4.
//
// Same dataflow, LDS images, operands and epilogue as attention_asm72.hip (read that file's header first); what differs:
//   * a workgroup is 4 waves x 128 query rows = 512 rows (four 32-row query blocks per wave instead of two);
//   * a loop body of the generated stream (tools/gen_attn_asm.py::LayoutW / body_wide -> attention_asm72w_f0.inc) handles ONE
//     32-key half of a 64-key tile for the four blocks: the same 20 + 40 MFMAs, 64 exp2, 32 packs and 16 lane-row swaps per body
//     and wave, but every K fragment read from LDS feeds 4 MFMAs instead of 2 and every V^T fragment 8 instead of 4, and a
//     tile's LDS-DMA pieces and loader advances are spread over two bodies: 157-161 non-MFMA instructions per 1280 matrix cycles
//     instead of 188, half the LDS fragment traffic and half the LDS-DMA issue per flop.  O^T: 160 AGPRs, Q: 80, 252 VGPRs.
// Only the bounded body exists in this layout (the general running-reference body needs its max-chain temporaries where the fifth
// V^T fragment slot lives); the entry point takes it for bounded calls with Lq >= 1024 (attention_fwd.hip).
#include "attention_asm_wrap.h"
#include "attention_asm_regs.inc"

namespace osk_attn {
namespace {

constexpr int HDL = 72, NKS = 5;   // HDL: the head_dim of the LDS images / register layout; the tensors' head_dim is the template parameter HD

template <int HD>   // 72, or 64 (see attention_asm72.hip)
__global__ void __launch_bounds__(256, 1) attn_asm72w_kernel(const AttnParams p) {
  constexpr int ROWS = 512;                                    // query rows per workgroup
  constexpr int NU = 4;                                        // 32-row query blocks per wave
  constexpr int NW = 4;                                        // waves
  constexpr int NSLOT = OSK72W_NSLOT;                          // LDS-DMA slots per wave and tile
  static_assert(NSLOT == 3 && OSK72_NDB == 5, "generated geometry changed: update the wrapper");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const Work w = decode_work<ROWS>(p);
  const int lane = w.lane, wave = w.wave, hi = w.hi;
  float bound;   // the caller's score bound, or -- auto-dispatched pairs -- the one this (batch, head)'s operands imply (attention_params.h)
  if (!attn_auto_bound(p, w.b, w.h, true, bound)) return;

  // ---- LDS, ragged-tile mask, Q fragments with the bound in their padding dim, loader offsets and operands: as in attention_asm72.hip
  clear_lds<OSK72_SMEM, NW>(smem, w.tid);
  __syncthreads();
  lds_ones_rows<OSK72_VOFF0, OSK72_VTILE, HDL>(smem, w.tid);
  lds_const_chunk<OSK72_CONST_OFF, OSK72_KTILE>(smem, w.tid);
  const int last_valid = p.seg_len - (p.tps - 1) * 64;   // keys in the last tile of a segment (1..64)
  const KeyPart kp = key_part(p, w.tail, w.part, w.qb, last_valid < 64);   // the whole key axis, or one part of a split tail unit
  const bool ragged = kp.ragged;
  const unsigned maskval = ragged_mask72(lane, last_valid);
  lds_mask_first_tile<OSK72_VOFF0, HDL>(smem, w.tid, kp, maskval);
  __syncthreads();

  int qi[NU];
  osk_v4f qv[NU * NKS];
  load_q_bf16<HD, HDL, NKS, NU, ROWS>(p, w, qi, qv);
#pragma unroll
  for (int u = 0; u < NU; ++u)
    if (hi) qv[u * NKS + 4][0] = __uint_as_float((__float_as_uint(-bound) >> 16) & 0xFFFFu);

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
    OSK_AQ_IN_40_5(qv), OSK_AQ_IN_45_5(qv + 5), OSK_AQ_IN_50_5(qv + 10), OSK_AQ_IN_55_5(qv + 15)
  asm volatile(
#include "attention_asm72w_f0.inc"
      OSK72_OPERANDS : OSK72W_CLOBBERS);
  m_ref[0] = m_ref[1] = bound;

  // the O^T accumulators as values the compiler knows (acc_quads.h): outputs of an empty statement right behind the loop
  static_assert(OSK72W_AQ0 == 160 && OSK72W_AQ1 == 180 && OSK72W_AQ2 == 200 && OSK72W_AQ3 == 220 && OSK72W_AO_REGS == 160,
                "the generated loop's register map: the operand lists above and below bind exactly these AGPRs");
  osk_v4f ov[40];
  asm volatile("" : OSK_AQ_OUT_0_40(ov));

  store_row_blocks16<HD, NU, ROWS, false>(ov, m_ref, p, w);   // (the bound: the same reference point for every row)
}

}  // namespace

int launch_asm72w(const AttnParams& p, hipStream_t st) { return launch_kernel<attn_asm72w_kernel<72>>(OSK72_SMEM, p, st); }
int launch_asm64w(const AttnParams& p, hipStream_t st) { return launch_kernel<attn_asm72w_kernel<64>>(OSK72_SMEM, p, st); }

}  // namespace osk_attn
