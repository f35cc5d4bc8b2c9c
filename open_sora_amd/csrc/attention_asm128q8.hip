// Flash-attention forward for head_dim 128, gfx950, with BOTH products on the fp8 MFMA (opt-in fp8 mode, qk8).
//
// attention_asm128p8.hip with QK^T on v_mfma_f32_32x32x64_f8f6f4 as well: K arrives as OCP e4m3 from osk_k_pack_fp8 (one scale per
// (key batch, head), natural byte order, a segment's last key repeated up to the 64-key tile boundary) and Q becomes e4m3 HERE,
// in the prologue, with one scale per query row and head (a lane owns one query; the other half of its 128 dims sits in lane
// l ^ 32).  A 64-key tile's QK^T is 2 k-steps x 2 key halves x 2 query blocks = 8 MFMAs of 64 cycles where the bf16 body needs 36
// of 32; the K tile is ONE swizzled LDS image of 64 rows x 128 bytes (8 LDS-DMA instructions, 2 per wave).
//  * fragments: K (k-step ks, key half t2) = key row 32 t2 + l % 32, bytes 64 ks + 32 (l / 32) .. + 31 (two ds_read_b128);
//    Q (block u, k-step ks) = the same 32 dims of query l % 32 of the block, 8 AGPRs; 32 AGPRs of Q in all;
//  * dequantisation and reference max: the scores leave the MFMA raw; ONE v_fma_f32 per score, s = c raw - M with the lane's
//    c = q scale x K scale and M in a register, sits in the P.V shadows in front of the max chains.  No padding k-step (it would
//    be a third 64-cycle step), no packed-FP32 instruction; the rare path (M moves) shifts the pending scores and rescales O as
//    in the bf16-QK^T bodies, it just has no Q padding dim to rewrite;
//  * P.V, the V^T ring, the baked ones / key-validity row, tail split, kv_batches, segment jumps and the epilogue: those of
//    attention_asm128p8.hip.  Ragged segment-last tiles need no clamped K offsets: the packed K repeats the last key.
#include "attention_asm_wrap.h"
#include "attention_asm_regs.inc"

namespace osk_attn {
namespace {

constexpr int HD = 128, NKS = OSK128Q8_NKS, NDT = OSK128Q8_NDT, NU = 2, NW = 4, ROWS = 256, NSLOT = OSK128Q8N2_NSLOT;
constexpr int NSLOT_V = OSK128Q8N2_NSLOT_V, RP = OSK128Q8_RP, NVD = OSK128Q8_NVD;
static_assert(NKS == 2 && NDT == 5 && NSLOT == 2 && NSLOT_V == 3 && RP == 144 && NVD == 9 && OSK128Q8_NKD == 8 && OSK128Q8_KTILE == 8192,
              "generated geometry changed: update the wrapper");

__global__ void __launch_bounds__(256, 1) attn_asm128q8_kernel(const AttnParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const Work w = decode_work<ROWS>(p);
  const int lane = w.lane, wave = w.wave, hi = w.hi, l31 = w.l31, b = w.b, h = w.h;

  clear_lds<OSK128Q8_SMEM, NW>(smem, w.tid);
  // ragged last key tile of a segment: the packed K repeats the segment's last key behind it (finite scores); the
  // key-validity row of V^T comes baked from osk_v_transpose_fp8
  const int last_valid = p.seg_len - (p.tps - 1) * 64;
  const KeyPart kp = key_part(p, w.tail, w.part, w.qb, last_valid < 64);   // the whole key axis, or one part of a split tail unit
  const bool ragged = kp.ragged;
  __syncthreads();

  // ---- Q -> e4m3 fragments in AGPRs.  Per query row and head: qf = f32(q) (* sc unless pre-scaled), s_q = absmax(qf) / 448 (1.0
  //      for an all-zero row), bytes = e4m3(clamp(qf / s_q, +-448)), round to nearest even.  The lane holds dims 64 ks + 32 hi
  //      .. + 31 of its query (ks = 0, 1); lane l ^ 32 holds the other 64, so the absmax takes one half-wave swap.
  const int bkv = b % p.Bkv;
  const float k_sc = p.k_scale[bkv * p.H + h];
  int qi[NU];
  float cq[NU];
  osk_v4f qv[NU * 4];
#pragma unroll
  for (int u = 0; u < NU; ++u) {
    qi[u] = w.qb * ROWS + wave * 64 + u * 32 + l31;
    const int qc = qi[u] < p.Lq ? qi[u] : p.Lq - 1;
    const unsigned short* qrow = p.q + b * p.qbs + (int64_t)qc * p.qrs + h * HD;
    float f[NKS][32];
    float amax = 0.f;
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks)
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const uint4 s = *reinterpret_cast<const uint4*>(qrow + ks * 64 + hi * 32 + c * 8);
        unpack8(s, &f[ks][c * 8]);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          if (!p.q_prescaled) f[ks][c * 8 + j] *= p.sc;
          amax = fmaxf(amax, fabsf(f[ks][c * 8 + j]));
        }
      }
    const unsigned au = __float_as_uint(amax);
    auto sw_ = __builtin_amdgcn_permlane32_swap(au, au, false, false);
    amax = fmaxf(__uint_as_float(sw_[0]), __uint_as_float(sw_[1]));
    const float s_q = amax > 0.f ? amax / 448.0f : 1.0f;
    cq[u] = s_q * k_sc;
    // fragment (u, ks) = two quads: register w holds dims 64 ks + 32 hi + 4 w .. + 3, low byte first
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks)
#pragma unroll
      for (int w = 0; w < 8; ++w) {
        float g[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) g[e] = fminf(fmaxf(f[ks][w * 4 + e] / s_q, -448.0f), 448.0f);
        int r = 0;
        r = __builtin_amdgcn_cvt_pk_fp8_f32(g[0], g[1], r, false);
        r = __builtin_amdgcn_cvt_pk_fp8_f32(g[2], g[3], r, true);
        qv[u * 4 + ks * 2 + w / 4][w % 4] = __uint_as_float((unsigned)r);
      }
  }

  // ---- per-lane LDS-DMA source offsets (bytes): K instruction j = wave + 4 i moves key rows 8 j + lane / 8 of the tile; LDS
  //      position lane % 8 of a 128-byte row holds the 16-byte chunk (lane % 8) ^ ((row >> 1) & 7) of it;
  //      V^T instruction j = (3 - wave) + 4 i -> dim rows 16 j + lane / 4
  const int srow8 = lane >> 3, spos = lane & 7;
  unsigned koff[NSLOT], voff[NSLOT_V];
#pragma unroll
  for (int i = 0; i < NSLOT; ++i) {
    const int row = (wave + NW * i) * 8 + srow8;
    koff[i] = (unsigned)(row * 128 + ((spos ^ ((row >> 1) & 7)) << 4));
  }
  const unsigned lds_base = lds_address(smem);
  unsigned vf0, vf1;
  vt8_offsets<NW, NSLOT_V, NVD>(p, w, lds_base, voff, vf0, vf1);
  // K fragment (ks, half j of its 32 bytes): row l31 (+ 32 t2 as an immediate), logical chunk 4 ks + 2 hi + j
  const int sw = (l31 >> 1) & 7;
  unsigned fo[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) fo[j] = lds_base + l31 * 128 + (((4 * (j >> 1) + 2 * hi + (j & 1)) ^ sw) << 4);

  // K strides are bytes here (k8 [Bkv, H, seg_lp, 128] per segment; key_part() multiplies tiles by krs = 128)
  const uint64_t kbase = rfl64((uint64_t)(uintptr_t)(p.k8 + bkv * p.kbs + (int64_t)h * p.seg_lp * 128 + kp.k_off));
  const unsigned kstep = rfl(64u * 128u);
  const uint64_t kjump = rfl64((uint64_t)(p.kss - (int64_t)p.tps * 64 * 128));
  const unsigned kdst = rfl(lds_base + wave * 1024);
  const VLoader vl = vt_loader<RP, OSK128Q8_VOFF0, NW>(p, w, kp, p.vt8, bkv, lds_base);   // V^T strides are bytes here
  const unsigned tps = rfl((unsigned)kp.tps), nt = rfl((unsigned)kp.nt);
  const unsigned nvw = rfl(((NW - 1 - wave) + NW * (NSLOT_V - 1) < NVD ? (unsigned)NSLOT_V : (unsigned)(NSLOT_V - 1)) |
                           (ragged ? 0u : 1u << 8));

  float m_ref[2];
#define OSK128Q8_OPERANDS                                                                                             \
  : "=&v"(m_ref[0]), "=&v"(m_ref[1])                                                                                  \
  : "v"(koff[0]), "v"(koff[1]), "v"(voff[0]), "v"(voff[1]), "v"(voff[2]),                                             \
    "v"(fo[0]), "v"(fo[1]), "v"(fo[2]), "v"(fo[3]), "v"(vf0), "v"(vf1), "v"(cq[0]), "v"(cq[1]),                       \
    "s"(kbase), "s"(vl.base), "s"(kstep), "s"(kjump), "s"(vl.jump), "s"(tps), "s"(nt), "s"(kdst), "s"(vl.dst), "s"(nvw), \
    OSK_AQ_IN_40_8(qv)
  asm volatile(
#include "attention_asm128q8_n2_v0.inc"
      OSK128Q8_OPERANDS : OSK128Q8N2_CLOBBERS);

  // the O^T accumulators as values the compiler knows (acc_quads.h): outputs of an empty statement right behind the loop
  static_assert(OSK128Q8N2_AQ0 == 160 && OSK128Q8N2_AQ1 == 176 && OSK128Q8N2_A_END == 192 && OSK128Q8N2_AO_REGS == 160,
                "the generated loop's register map: the operand lists above and below bind exactly these AGPRs");
  osk_v4f ov[40];
  asm volatile("" : OSK_AQ_OUT_0_40(ov));

  // row 128 of O^T = sum_k P: row 0 of row tile 4 = lanes hi == 0, register 0
  store_row_tiles<HD, NDT, NU, 4, 0, ROWS>(ov, p.v_scale[bkv * p.H + h], m_ref, p, w, qi);
}

}  // namespace

int launch_asm128q8(const AttnParams& p, hipStream_t st) { return launch_kernel<attn_asm128q8_kernel>(OSK128Q8_SMEM, p, st); }

}  // namespace osk_attn
