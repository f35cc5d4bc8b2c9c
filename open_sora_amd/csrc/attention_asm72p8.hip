// Flash-attention forward for head_dim 72, gfx950, with the P.V product on the fp8 MFMA (opt-in fp8 mode): the
// head_dim-72 twin of attention_asm128p8.hip (see there): 4 waves x 64 query rows, QK^T and the softmax bookkeeping of
// attention_asm72.hip, P and V^T as e4m3, one v_mfma_f32_32x32x64_f8f6f4 per O^T row tile (3 x 64 cycles instead of
// 12 x 32), V^T with RP = 80 rows per head from osk_v_transpose_fp8 (72 dims, the ones / key-validity row 72, zero rows).
#include "attention_asm_wrap.h"
#include "attention_asm_regs.inc"

namespace osk_attn {
namespace {

constexpr int HD = 72, NKS = 5, NDT = 3, ROWS = 256;
constexpr int NSLOT_V = OSK72P8N2_NSLOT_V, RP = OSK72P8_RP, NVD = OSK72P8_NVD;
static_assert(NSLOT_V == 2 && RP == 80 && NVD == 5, "generated geometry changed: update the wrapper");

template <int NU>
__global__ void __launch_bounds__(NU == 2 ? 256 : 512, NU == 2 ? 1 : 2) attn_asm72p8_kernel(const AttnParams p) {
  constexpr int NW = 8 / NU;                                   // waves per workgroup
  static_assert(NU == 2, "the fp8 P.V variant exists in the 4 waves x 64 rows layout only");
  constexpr int NSLOT = OSK72P8N2_NSLOT;  // LDS-DMA slots per wave and tile
  static_assert(NSLOT == 3, "generated geometry changed: update the wrapper");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const Work w = decode_work<ROWS>(p);
  const int wave = w.wave;

  // ---- LDS: zero, constant chunk {1.0, 0 x 7} = K's padding dims 72..79
  clear_lds<OSK72P8_SMEM, NW>(smem, w.tid);
  __syncthreads();
  lds_const_chunk<OSK72P8_CONST_OFF, OSK72P8_KTILE>(smem, w.tid);
  // ragged last key tile of a segment: K rows past the segment re-fetch its last key (finite scores); the key-validity
  // row of V^T comes baked from osk_v_transpose_fp8
  const int last_valid = p.seg_len - (p.tps - 1) * 64;
  const KeyPart kp = key_part(p, w.tail, w.part, w.qb, last_valid < 64);
  const bool ragged = kp.ragged;
  __syncthreads();

  int qi[NU];
  osk_v4f qv[NU * NKS];
  load_q_bf16<HD, HD, NKS, NU, ROWS>(p, w, qi, qv);

  const unsigned lds_base = lds_address(smem);
  unsigned koff[NSLOT], koffL[NSLOT], voff8[NSLOT_V], vf0, vf1;
  k_offsets72<NW, NSLOT>(p, w, last_valid, koff, koffL);
  vt8_offsets<NW, NSLOT_V, NVD>(p, w, lds_base, voff8, vf0, vf1);
  unsigned fo[4], kc[2];
  k_frag_addrs(w, lds_base, fo);
  k_col_addrs72<OSK72P8_CONST_OFF>(w, lds_base, kc);

  const int bkv = w.b % p.Bkv;   // key / value batch of this query batch
  const KLoader kl = k_loader<HD>(p, w, kp, bkv, lds_base);
  const VLoader vl = vt_loader<RP, OSK72P8_VOFF0, NW>(p, w, kp, p.vt8, bkv, lds_base);   // V^T strides are bytes here
  const unsigned tps = rfl((unsigned)kp.tps), nt = rfl((unsigned)kp.nt);
  // valid loader slots of this wave: the last one only where its instruction index is < 9
  const unsigned nkw = rfl(wave + NW * (NSLOT - 1) < 9 ? (unsigned)NSLOT : (unsigned)(NSLOT - 1));
  const unsigned nvw = rfl(((NW - 1 - wave) + NW * (NSLOT_V - 1) < NVD ? (unsigned)NSLOT_V : (unsigned)(NSLOT_V - 1)) |
                           (ragged ? 0u : 1u << 8));

  float m_ref[2];
#define OSK72P8_OPERANDS                                                                                              \
  : "=&v"(m_ref[0]), "=&v"(m_ref[1])                                                                                  \
  : "v"(koff[0]), "v"(koff[1]), "v"(koff[2]), "v"(voff8[0]), "v"(voff8[1]), "v"(fo[0]), "v"(fo[1]),                   \
    "v"(fo[2]), "v"(fo[3]), "v"(kc[0]), "v"(kc[1]), "v"(koffL[0]), "v"(koffL[1]), "v"(koffL[2]), "v"(vf0), "v"(vf1),  \
    "s"(kl.base), "s"(vl.base),                                                                                       \
    "s"(kl.step), "s"(kl.jump), "s"(vl.jump), "s"(tps), "s"(nt), "s"(kl.dst), "s"(vl.dst), "s"(nkw), "s"(nvw),        \
    OSK_AQ_IN_24_5(qv), OSK_AQ_IN_29_5(qv + 5)
  asm volatile(
#include "attention_asm72p8_n2_v0.inc"
      OSK72P8_OPERANDS : OSK72P8N2_CLOBBERS);

  // the O^T accumulators as values the compiler knows (acc_quads.h): outputs of an empty statement right behind the loop
  static_assert(OSK72P8N2_AQ0 == 96 && OSK72P8N2_AQ1 == 116 && OSK72P8N2_AO_REGS == 96,
                "the generated loop's register map: the operand lists above and below bind exactly these AGPRs");
  osk_v4f ov[24];
  asm volatile("" : OSK_AQ_OUT_0_24(ov));
  // row 72 of O^T = sum_k P: lanes hi == 0, register (8 & 3) + 4 (8 >> 3) = 4 of row tile 2
  store_row_tiles<HD, NDT, NU, 2, 4, ROWS>(ov, p.v_scale[bkv * p.H + w.h], m_ref, p, w, qi);
}

}  // namespace

int launch_asm72p8(const AttnParams& p, hipStream_t st) { return launch_kernel<attn_asm72p8_kernel<2>>(OSK72P8_SMEM, p, st); }

}  // namespace osk_attn
