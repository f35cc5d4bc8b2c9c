// Flash-attention forward for head_dim 128, gfx950, with the P.V product on the fp8 MFMA (opt-in fp8 mode).
//
// attention_asm128.hip with one change of arithmetic: P (<= 2^8 by construction) and V^T are OCP e4m3, and a 64-key tile's
// P.V is ONE v_mfma_f32_32x32x64_f8f6f4 per O^T row tile (5 x 64 cycles instead of 20 x 32).  A lane's 32 P values of
// a tile (two 32 x 32 score tiles x 16 accumulator registers) are exactly one fp8 B operand; the byte order that falls
// out of the accumulator layout -- byte t2*16 + j*4 + i of half-wave hi <-> key 32 t2 + 8 j + 4 hi + i -- is baked into
// the V^T rows by osk_v_transpose_fp8, which also quantises V with one scale per (batch, head) and appends the ones /
// key-validity row and zero rows (RP = 144 rows per head), so the kernel keeps no ones row of its own.  QK^T, the
// softmax bookkeeping and the output stay as in the bf16 kernel; O is multiplied by the V scale in the epilogue.
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

constexpr int HD = 128, NKS = OSK128P8_NKS, NDT = OSK128P8_NDT, NU = 2, NW = 4, ROWS = 256, NSLOT = OSK128P8N2_NSLOT;
constexpr int NSLOT_V = OSK128P8N2_NSLOT_V, RP = OSK128P8_RP, NVD = OSK128P8_NVD;
static_assert(NKS == 9 && NDT == 5 && NSLOT == 4 && NSLOT_V == 3 && RP == 144 && NVD == 9, "generated geometry changed: update the wrapper");

__global__ void __launch_bounds__(256, 1) attn_asm128p8_kernel(const AttnParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const Work w = decode_work<ROWS>(p);
  const int wave = w.wave;

  clear_lds<OSK128P8_SMEM, NW>(smem, w.tid);
  // ragged last key tile of a segment: K rows past the segment re-fetch its last key (finite scores); the key-validity
  // row of V^T comes baked from osk_v_transpose_fp8
  const int last_valid = p.seg_len - (p.tps - 1) * 64;
  const KeyPart kp = key_part(p, w.tail, w.part, w.qb, last_valid < 64);   // the whole key axis, or one part of a split tail unit
  const bool ragged = kp.ragged;
  __syncthreads();

  // ---- Q fragments; k-step 8 = padding (zero; dim 128 receives -M in the asm)
  int qi[NU];
  osk_v4f qv[NU * NKS];
  load_q_bf16<HD, HD, NKS, NU, ROWS>(p, w, qi, qv);

  const unsigned lds_base = lds_address(smem);
  unsigned koff[NSLOT], koffL[NSLOT], voff[NSLOT_V], vf0, vf1;
  k_offsets128<NW, NSLOT>(p, w, last_valid, koff, koffL);
  vt8_offsets<NW, NSLOT_V, NVD>(p, w, lds_base, voff, vf0, vf1);
  unsigned fo[4];
  k_frag_addrs(w, lds_base, fo);

  const int bkv = w.b % p.Bkv;
  const KLoader kl = k_loader<HD>(p, w, kp, bkv, lds_base);
  const VLoader vl = vt_loader<RP, OSK128P8_VOFF0, NW>(p, w, kp, p.vt8, bkv, lds_base);   // V^T strides are bytes here
  const unsigned tps = rfl((unsigned)kp.tps), nt = rfl((unsigned)kp.nt);
  const unsigned nvw = rfl(((NW - 1 - wave) + NW * (NSLOT_V - 1) < NVD ? (unsigned)NSLOT_V : (unsigned)(NSLOT_V - 1)) |
                           (ragged ? 0u : 1u << 8));

  float m_ref[2];
#define OSK128P8_OPERANDS                                                                                             \
  : "=&v"(m_ref[0]), "=&v"(m_ref[1])                                                                                  \
  : "v"(koff[0]), "v"(koff[1]), "v"(koff[2]), "v"(koff[3]), "v"(voff[0]), "v"(voff[1]), "v"(voff[2]),                 \
    "v"(fo[0]), "v"(fo[1]), "v"(fo[2]), "v"(fo[3]), "v"(koffL[0]), "v"(koffL[1]), "v"(koffL[2]), "v"(koffL[3]),       \
    "v"(vf0), "v"(vf1), "s"(kl.base), "s"(vl.base),                                                                   \
    "s"(kl.step), "s"(kl.jump), "s"(vl.jump), "s"(tps), "s"(nt), "s"(kl.dst), "s"(vl.dst), "s"(nvw),                  \
    OSK_AQ_IN_40_5(qv), OSK_AQ_IN_45_4(qv + 5), OSK_AQ_IN_49_5(qv + 9), OSK_AQ_IN_54_4(qv + 14)
  asm volatile(
#include "attention_asm128p8_n2_v0.inc"
      OSK128P8_OPERANDS : OSK128P8N2_CLOBBERS);

  // the O^T accumulators as values the compiler knows (acc_quads.h): outputs of an empty statement right behind the loop
  static_assert(OSK128P8N2_AQ0 == 160 && OSK128P8N2_AQ1 == 196 && OSK128P8N2_AO_REGS == 160,
                "the generated loop's register map: the operand lists above and below bind exactly these AGPRs");
  osk_v4f ov[40];
  asm volatile("" : OSK_AQ_OUT_0_40(ov));
  // row 128 of O^T = sum_k P: row 0 of row tile 4 = lanes hi == 0, register 0
  store_row_tiles<HD, NDT, NU, 4, 0, ROWS>(ov, p.v_scale[bkv * p.H + w.h], m_ref, p, w, qi);
}

}  // namespace

int launch_asm128p8(const AttnParams& p, hipStream_t st) { return launch_kernel<attn_asm128p8_kernel>(OSK128P8_SMEM, p, st); }

}  // namespace osk_attn
