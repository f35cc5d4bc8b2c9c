// What the wrappers of the hand-scheduled attention loops (attention_asm{72,72w,72p8,128,128p8,128q8}.hip) have in common: the work
// decode, LDS set-up, Q fragments, loader offsets and operands in front of a loop statement, and the two epilogue forms behind it.
// Plain device functions with compile-time geometry; every kernel keeps its own geometry constants, operand list, loop statement,
// register-map assert and accumulator binding in its own file, next to the loop they describe.
// The helpers take the work unit by value and the launch parameters as a __restrict__ reference (nothing else points at a kernel's
// parameter block).  The compiler simplifies a helper before it inlines it; with plain references the kernels came out 1 - 8 % longer
// (the epilogues re-read the parameters behind their stores), with these within 1 % of the hand-inlined code: the instruction counts
// are in profiles/attn_wrap_ab.md.
#pragma once
#include "acc_quads.h"
#include "attention_params.h"

namespace osk_attn {

// ---- a workgroup's lane geometry and work unit: ROWS query rows of (batch b, head h), or one key part of a split tail unit
struct Work {
  int tid, lane, wave, hi, l31;   // wave is wave-uniform; hi = lane / 32, l31 = lane % 32
  int bh, qb, part, tail_unit, b, h;
  bool tail;
};
template <int ROWS>
OSK_DEV Work decode_work(const AttnParams& __restrict__ p) {
  Work w;
  w.tid = threadIdx.x;
  w.lane = w.tid & 63;
  w.wave = __builtin_amdgcn_readfirstlane(w.tid >> 6);
  w.hi = w.lane >> 5;
  w.l31 = w.lane & 31;
  w.tail = block_to_work_split(p, (p.Lq + ROWS - 1) / ROWS, w.bh, w.qb, w.part, w.tail_unit);
  w.b = w.bh / p.H;
  w.h = w.bh - w.b * p.H;
  return w;
}

// LDS: zero (a tile slot that is never filled must hold finite data).  No barrier: the caller places it.
template <int SMEM, int NW>
OSK_DEV void clear_lds(unsigned char* smem, int tid) {
  for (int i = tid; i < SMEM / 16; i += 64 * NW) reinterpret_cast<uint4*>(smem)[i] = make_uint4(0, 0, 0, 0);
}
OSK_DEV unsigned lds_address(unsigned char* smem) { return (unsigned)(uintptr_t)(__attribute__((address_space(3))) unsigned char*)smem; }

// ones row (LDS row ROW of the bf16 V^T tile: the softmax denominator rides in the P.V product) of both V^T ring slots
template <int VOFF0, int VTILE, int ROW>
OSK_DEV void lds_ones_rows(unsigned char* smem, int tid) {
  if (tid < 64) {
    const int slot = tid >> 5;
    reinterpret_cast<unsigned*>(smem + VOFF0 + slot * VTILE + ROW * 128)[tid & 31] = 0x3F803F80u;
  }
}
// head_dim 72: constant chunk {1.0, 0 x 7} = K's padding dims 72..79
template <int CONST_OFF, int KTILE>
OSK_DEV void lds_const_chunk(unsigned char* smem, int tid) {
  if (tid == 64 || tid == 65)  // one copy per K ring slot, KTILE apart (the slot is an immediate offset in the asm)
    *reinterpret_cast<unsigned*>(smem + CONST_OFF + (tid - 64) * KTILE) = 0x00003F80u;
}
// head_dim 72, bf16 V^T: the ones row of a ragged tile as a key-validity mask, in the V^T tile's baked key order
OSK_DEV unsigned ragged_mask72(int lane, int last_valid) {
  unsigned maskval = 0;
  if (lane < 32) {
    // dword `lane` of LDS row 72: 16-byte position lane / 4 holds logical chunk c = (lane / 4) ^ ((72 >> 1) & 7) of the swizzled
    // 128-byte row image; chunk c of the V^T tile = 32-key half c / 4, lane row c % 4, whose 8 keys (baked by
    // osk_v_transpose_bf16 for this head_dim) are PV16_KEYS[c % 4] (tools/gen_attn_asm.py)
    const int c = (lane >> 2) ^ ((72 >> 1) & 7), e0 = (lane & 3) * 2;
    auto key_of = [](int c_, int e_) {
      const int r_ = c_ & 3;   // lane row: keys {0-3, 8-11}, {16-19, 24-27}, {4-7, 12-15}, {20-23, 28-31}
      return 32 * (c_ >> 2) + ((r_ & 1) << 4) + ((r_ >> 1) << 2) + ((e_ >> 2) << 3) + (e_ & 3);
    };
    maskval = (key_of(c, e0) < last_valid ? 0x3F80u : 0u) | (key_of(c, e0 + 1) < last_valid ? 0x3F800000u : 0u);
  }
  return maskval;
}

// ---- bf16 Q fragments, pre-scaled by scale*log2(e), as the quads the loop statement binds to its AGPRs (u-major, k-step, 4 words).
// HD: the tensors' head_dim; HDL: that of the register layout, whose NKS k-steps of 16 dims end in padding (zero here; the
// reference max goes there).  Rows past Lq re-read row Lq - 1; qi[u] is the lane's row of query block u, not clamped.
template <int HD, int HDL, int NKS, int NU, int ROWS>
OSK_DEV void load_q_bf16(const AttnParams& __restrict__ p, const Work w, int (&qi)[NU], osk_v4f (&qv)[NU * NKS]) {
#pragma unroll
  for (int u = 0; u < NU; ++u) {
    qi[u] = w.qb * ROWS + w.wave * (32 * NU) + u * 32 + w.l31;
    const int qc = qi[u] < p.Lq ? qi[u] : p.Lq - 1;
    const unsigned short* qrow = p.q + w.b * p.qbs + (int64_t)qc * p.qrs + w.h * HD;
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) {
      uint4 s = make_uint4(0, 0, 0, 0);
      if (ks * 16 < HDL) {
        const int e0 = ks * 16 + w.hi * 8;
        if (e0 < HD) s = *reinterpret_cast<const uint4*>(qrow + e0);
        if (!p.q_prescaled) {  // fold scale*log2(e) in here (one extra bf16 rounding of q); see osk.h
          float f[8];
          unpack8(s, f);
#pragma unroll
          for (int j = 0; j < 8; ++j) f[j] *= p.sc;
          s = pack8(f);
        }
      }
      // Q fragments as VALUES: quad ks of block u; the loop statement takes them as inputs in their fixed AGPRs (acc_quads.h), so the
      // compiler writes them there itself and knows they are live until the loop has read them
      qv[u * NKS + ks] = osk_v4f{__uint_as_float(s.x), __uint_as_float(s.y), __uint_as_float(s.z), __uint_as_float(s.w)};
    }
  }
}

// ---- per-lane LDS-DMA source offsets (bytes from the loader's tile base) of this wave's instruction slots.  koffL: the same for
// the ragged last tile of a segment (last_valid < 64 keys), where rows past the segment re-fetch its last key (finite scores).
// head_dim 72: K instruction j = wave + NW i moves key rows 8 j + lane / 8 of the swizzled 64-dim image; j = 8: the 8-dim column
// image (dims 64..71 of 64 keys); a slot past it stays 0
template <int NW, int NSLOT>
OSK_DEV void k_offsets72(const AttnParams& __restrict__ p, const Work w, int last_valid, unsigned (&koff)[NSLOT], unsigned (&koffL)[NSLOT]) {
  const int srow8 = w.lane >> 3, spos = w.lane & 7;
#pragma unroll
  for (int i = 0; i < NSLOT; ++i) {
    const int j = w.wave + NW * i;
    unsigned o = 0, oL = 0;
    if (j < 8) {
      const int row = j * 8 + srow8;
      const int rowL = row < last_valid ? row : last_valid - 1;
      const int ch = (spos ^ ((row >> 1) & 7)) << 3;
      o = (unsigned)(((int64_t)row * p.krs + ch) * 2);
      oL = (unsigned)(((int64_t)rowL * p.krs + ch) * 2);
    } else if (j == 8) {
      const int rowL = w.lane < last_valid ? w.lane : last_valid - 1;
      o = (unsigned)(((int64_t)w.lane * p.krs + 64) * 2);
      oL = (unsigned)(((int64_t)rowL * p.krs + 64) * 2);
    }
    koff[i] = o;
    koffL[i] = oL;
  }
}
// head_dim 128: K instruction j = wave + NW i -> image j / 8 (dims 0..63, 64..127), key rows 8 (j % 8) + lane / 8
template <int NW, int NSLOT>
OSK_DEV void k_offsets128(const AttnParams& __restrict__ p, const Work w, int last_valid, unsigned (&koff)[NSLOT], unsigned (&koffL)[NSLOT]) {
  const int srow8 = w.lane >> 3, spos = w.lane & 7;
#pragma unroll
  for (int i = 0; i < NSLOT; ++i) {
    const int j = w.wave + NW * i;
    const int img = j >> 3, row = (j & 7) * 8 + srow8;
    const int rowL = row < last_valid ? row : last_valid - 1;
    const int ch = img * 64 + ((spos ^ ((row >> 1) & 7)) << 3);
    koff[i] = (unsigned)(((int64_t)row * p.krs + ch) * 2);
    koffL[i] = (unsigned)(((int64_t)rowL * p.krs + ch) * 2);
  }
}
// bf16 V^T: instruction j = (NW - 1 - wave) + NW i moves dim rows 8 j + lane / 8 (same swizzled 128-byte-row image as K); a slot
// past the head's HD / 8 instructions stays 0
template <int HD, int NW, int NSLOT>
OSK_DEV void vt_offsets(const AttnParams& __restrict__ p, const Work w, unsigned (&voff)[NSLOT]) {
  const int srow8 = w.lane >> 3, spos = w.lane & 7;
#pragma unroll
  for (int i = 0; i < NSLOT; ++i) {
    const int jv = (NW - 1 - w.wave) + NW * i;
    unsigned ov = 0;
    // (head_dim 128: every slot has its instruction, jv <= 15; the compiler does not know the range of `wave` and would keep the
    //  compare and select -- 16 instructions per kernel -- so the first term says it at compile time)
    if (NW * NSLOT <= HD / 8 || jv < HD / 8) {
      const int d = jv * 8 + srow8;
      ov = (unsigned)(((int64_t)d * p.seg_lp + ((spos ^ ((d >> 1) & 7)) << 3)) * 2);
    }
    voff[i] = ov;
  }
}
// e4m3 V^T (64-byte rows, NVD instructions of 16 rows per head): instruction j = (NW - 1 - wave) + NW i moves rows [16 j, 16 j + 16);
// LDS position lane % 4 of a row holds the 16-byte chunk (lane % 4) ^ ((row >> 2) & 3) of it
// (64-byte rows: rows r, r + 4, r + 8, r + 12 share a 16-bank group, so the swizzle must tell THOSE apart).
// vf0, vf1: the V^T fragment of a row tile: row l31, the 32-byte half hi of its 64 keys = logical chunks 2 hi, 2 hi + 1
template <int NW, int NSLOT_V, int NVD>
OSK_DEV void vt8_offsets(const AttnParams& __restrict__ p, const Work w, unsigned lds_base, unsigned (&voff8)[NSLOT_V], unsigned& vf0, unsigned& vf1) {
#pragma unroll
  for (int i = 0; i < NSLOT_V; ++i) {
    const int jv = (NW - 1 - w.wave) + NW * i;
    const int row = (jv < NVD ? jv : 0) * 16 + (w.lane >> 2);
    voff8[i] = (unsigned)((int64_t)row * p.seg_lp + (((w.lane & 3) ^ ((row >> 2) & 3)) << 4));
  }
  const int sw4 = (w.l31 >> 2) & 3;
  vf0 = lds_base + w.l31 * 64 + (((2 * w.hi) ^ sw4) << 4);
  vf1 = lds_base + w.l31 * 64 + (((2 * w.hi + 1) ^ sw4) << 4);
}
// bf16 K fragments of the 32x32x16 QK^T product: row l31 of a swizzled 64-dim image, chunk 2 j + hi (k-step j of the image)
OSK_DEV void k_frag_addrs(const Work w, unsigned lds_base, unsigned (&fo)[4]) {
  const int sw = (w.l31 >> 1) & 7;
#pragma unroll
  for (int j = 0; j < 4; ++j) fo[j] = lds_base + w.l31 * 128 + (((2 * j + w.hi) ^ sw) << 4);
}

// head_dim 72: the fifth QK^T k-step (dims 64..79) reads, in lanes 0..31, the 8-dim column image of key half t2 and, in lanes 32..63,
// the constant chunk; ring slot 1 = + KTILE (immediate), for the column image and the constant chunk alike
template <int CONST_OFF>
OSK_DEV void k_col_addrs72(const Work w, unsigned lds_base, unsigned (&kc)[2]) {
#pragma unroll
  for (int t2 = 0; t2 < 2; ++t2) kc[t2] = w.hi ? lds_base + CONST_OFF : lds_base + 8192 + t2 * 512 + w.l31 * 16;
}
// head_dim 72, bf16 V^T fragments of the 16x16x32 P.V product: lane (row r4 = lane / 16, dim l15 = lane % 16 of a 16-row block) reads
// chunk 4 t2 + r4 of its row (+ block and ring-slot immediates in the asm); same swizzled 128-byte-row image as K
OSK_DEV void vt_frag_addrs72(const Work w, unsigned lds_base, unsigned (&vo)[2]) {
  const int l15 = w.lane & 15, r4 = w.lane >> 4;
#pragma unroll
  for (int t2 = 0; t2 < 2; ++t2) vo[t2] = lds_base + l15 * 128 + (((4 * t2 + r4) ^ ((l15 >> 1) & 7)) << 4);
}
// bf16 V^T: tile 0 itself is ragged (no loop body precedes it to write the mask): the validity mask into the ones row ROW of slot 0
template <int VOFF0, int ROW>
OSK_DEV void lds_mask_first_tile(unsigned char* smem, int tid, const KeyPart& kp, unsigned maskval) {
  if (kp.ragged && kp.tps == 1 && tid < 32) reinterpret_cast<unsigned*>(smem + VOFF0 + ROW * 128)[tid] = maskval;
}
// head_dim 72, bf16 V^T: the loader's slot word: valid V^T slots of this wave (the last one only where its instruction exists: index
// < HD / 8), bit 8 = no ragged tile, bit 9 = this wave writes the ragged tile's mask; valid K slots << 16 (head_dim 64: no column image)
template <int HD, int NW, int NSLOT>
OSK_DEV unsigned loader_slots72(int wave, bool ragged) {
  const unsigned nkw = rfl(wave + NW * (NSLOT - 1) < HD / 8 ? (unsigned)NSLOT : (unsigned)(NSLOT - 1));
  const unsigned nvw = rfl(((NW - 1 - wave) + NW * (NSLOT - 1) < HD / 8 ? (unsigned)NSLOT : (unsigned)(NSLOT - 1)) |
                           (ragged ? 0u : 1u << 8) | ((ragged && wave == 0) ? 1u << 9 : 0u));
  return rfl(nvw | (nkw << 16));
}

// ---- the loader's scalar operands (wave-uniform: SGPRs).  K as bf16 rows of krs elements; V^T rows of seg_lp elements of VT
// (bf16, or e4m3: strides in bytes), VROWS of them per head
struct KLoader {
  uint64_t base, jump;   // first tile of this part; from a segment's last tile to the next segment's first
  unsigned step, dst;    // one tile; this wave's first LDS row block
};
struct VLoader {
  uint64_t base, jump;
  unsigned dst;
};
template <int HD>
OSK_DEV KLoader k_loader(const AttnParams& __restrict__ p, const Work w, const KeyPart& kp, int bkv, unsigned lds_base) {
  KLoader r;
  r.base = rfl64((uint64_t)(uintptr_t)(p.k + bkv * p.kbs + w.h * HD + kp.k_off));
  r.step = rfl((unsigned)(128 * p.krs));
  r.jump = rfl64((uint64_t)((p.kss - (int64_t)p.tps * 64 * p.krs) * 2));
  r.dst = rfl(lds_base + w.wave * 1024);
  return r;
}
template <int VROWS, int VOFF0, int NW, typename VT>
OSK_DEV VLoader vt_loader(const AttnParams& __restrict__ p, const Work w, const KeyPart& kp, const VT* vt, int bkv, unsigned lds_base) {
  VLoader r;
  r.base = rfl64((uint64_t)(uintptr_t)(vt + (int64_t)(bkv * p.H + w.h) * VROWS * p.seg_lp + kp.v_off));
  r.jump = rfl64((uint64_t)((p.vtss - (int64_t)p.tps * 64) * (int)sizeof(VT)));
  r.dst = rfl(lds_base + VOFF0 + (NW - 1 - w.wave) * 1024);
  return r;
}

// ---- epilogue, 32-query row-tile form: O^T out of the AGPRs (row tile (u, d) = quads 4 (u NDT + d) ..: lane = query l31, dims
// 32 d + 8 qd + 4 hi + i in register 4 qd + i), normalise by the accumulator row that holds sum_k P (register SUM_REG of row tile
// SUM_TILE, lanes hi == 0), store.  inv_scale: 1, or the e4m3 scale of V (1 / sum(P) and the scale in one factor).
template <int HD, int NDT, int NU, int SUM_TILE, int SUM_REG, int ROWS>
OSK_DEV void store_row_tiles(const osk_v4f (&ov)[NU * NDT * 4], float inv_scale, const float (&m_ref)[NU], const AttnParams& __restrict__ p,
                             const Work w, const int (&qi)[NU]) {
#pragma unroll
  for (int u = 0; u < NU; ++u) {
    float o[NDT][16];
#pragma unroll
    for (int d = 0; d < NDT; ++d) {
#pragma unroll
      for (int i = 0; i < 16; ++i)   // in place, in program order
        asm volatile("v_accvgpr_read_b32 %0, %1" : "=v"(o[d][i]) : "a"(ov[(u * NDT + d) * 4 + i / 4][i % 4]));
    }
    const unsigned lu = __float_as_uint(o[SUM_TILE][SUM_REG]);
    auto sw2 = __builtin_amdgcn_permlane32_swap(lu, lu, false, false);
    const float l_tot = __uint_as_float(sw2[0]);
    const float inv = inv_scale / l_tot;
    if (w.tail) {
      // part of a split tail unit: normalised partial O (f32) + log2-domain LSE -> workspace (attn_merge_kernel)
      if (qi[u] < p.Lq) {
        const int64_t slot = ((int64_t)w.tail_unit * p.tail_split + w.part) * ROWS + (w.wave * (32 * NU) + u * 32 + w.l31);
        float* wo = p.ws_o + slot * HD;
#pragma unroll
        for (int d = 0; d < (HD + 31) / 32; ++d) {
#pragma unroll
          for (int qd = 0; qd < 4; ++qd) {
            const int d0 = d * 32 + qd * 8 + w.hi * 4;
            if (d0 < HD)
              *reinterpret_cast<float4*>(wo + d0) = make_float4(o[d][qd * 4 + 0] * inv, o[d][qd * 4 + 1] * inv,
                                                                 o[d][qd * 4 + 2] * inv, o[d][qd * 4 + 3] * inv);
          }
        }
        if (w.hi == 0) p.ws_lse[slot] = m_ref[u] + __builtin_amdgcn_logf(l_tot);
      }
    } else if (qi[u] < p.Lq) {
      unsigned short* orow = p.out + w.b * p.obs + (int64_t)qi[u] * p.ors + w.h * HD;
#pragma unroll
      for (int d = 0; d < (HD + 31) / 32; ++d) {
#pragma unroll
        for (int qd = 0; qd < 4; ++qd) {
          const int d0 = d * 32 + qd * 8 + w.hi * 4;
          if (d0 < HD) {
            uint2 w2;
            w2.x = pack_bf16x2(o[d][qd * 4 + 0] * inv, o[d][qd * 4 + 1] * inv);
            w2.y = pack_bf16x2(o[d][qd * 4 + 2] * inv, o[d][qd * 4 + 3] * inv);
            *reinterpret_cast<uint2*>(orow + d0) = w2;
          }
        }
      }
      if (p.lse && w.hi == 0)
        p.lse[(int64_t)w.bh * p.Lq + qi[u]] = (m_ref[u] + __builtin_amdgcn_logf(l_tot)) * 0.6931471805599453f;
    }
  }
}

// ---- epilogue, 16-query block form (head_dim 72, bf16 P.V on the 16x16x32 MFMA: 5 row blocks of 16): O^T out of the AGPRs -- per
// 16-query block (u, half): lane = query l15, dims 16 db + 4 r4 + i in register 4 db + i -- normalise by accumulator row 72 (sum of
// P: block 4, lane row 2, register 0), store.  ROW_REF: every query has its own reference max m_ref[u], in the SCORE layout (lane =
// query lane % 32 of block u); otherwise m_ref[0] is the reference point of every row (a bounded body)
template <int HD, int NU, int ROWS, bool ROW_REF>
OSK_DEV void store_row_blocks16(const osk_v4f (&ov)[NU * 10], const float* m_ref, const AttnParams& __restrict__ p, const Work w) {
  const int l15 = w.lane & 15, r4 = w.lane >> 4;
#pragma unroll
  for (int u = 0; u < NU; ++u) {
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      float o[20];
#pragma unroll
      for (int i = 0; i < 20; ++i)   // block (u, half) = registers 20 (2 u + half) ..: in place, in program order
        asm volatile("v_accvgpr_read_b32 %0, %1" : "=v"(o[i]) : "a"(ov[(u * 2 + half) * 5 + i / 4][i % 4]));
      const float l_tot = __shfl(o[16], 32 + l15, 64);
      const float inv = 1.0f / l_tot;
      float mq = m_ref[0];
      if constexpr (ROW_REF) mq = __shfl(m_ref[u], half * 16 + l15, 64);   // fetch this lane's query's
      const int wrow = w.wave * (32 * NU) + u * 32 + half * 16 + l15;   // row inside the workgroup's ROWS
      const int qrow = w.qb * ROWS + wrow;
      if (qrow >= p.Lq) continue;
      if (w.tail) {
        // part of a split tail unit: normalised partial O (f32) + log2-domain LSE -> workspace (attn_merge_kernel)
        const int64_t slot = ((int64_t)w.tail_unit * p.tail_split + w.part) * ROWS + wrow;
        float* wo = p.ws_o + slot * HD;
#pragma unroll
        for (int db = 0; db < 5; ++db) {
          const int d0 = db * 16 + r4 * 4;
          if (d0 < HD)
            *reinterpret_cast<float4*>(wo + d0) = make_float4(o[db * 4 + 0] * inv, o[db * 4 + 1] * inv, o[db * 4 + 2] * inv, o[db * 4 + 3] * inv);
        }
        if (r4 == 0) p.ws_lse[slot] = mq + __builtin_amdgcn_logf(l_tot);
      } else {
        unsigned short* orow = p.out + w.b * p.obs + (int64_t)qrow * p.ors + w.h * HD;
#pragma unroll
        for (int db = 0; db < 5; ++db) {
          const int d0 = db * 16 + r4 * 4;
          if (d0 < HD) {
            uint2 w2;
            w2.x = pack_bf16x2(o[db * 4 + 0] * inv, o[db * 4 + 1] * inv);
            w2.y = pack_bf16x2(o[db * 4 + 2] * inv, o[db * 4 + 3] * inv);
            *reinterpret_cast<uint2*>(orow + d0) = w2;
          }
        }
        if (p.lse && r4 == 0)
          p.lse[(int64_t)w.bh * p.Lq + qrow] = (mq + __builtin_amdgcn_logf(l_tot)) * 0.6931471805599453f;
      }
    }
  }
}

// host: one launch of 256 threads per work unit (and per key part of a split tail unit).  The kernel is a template ARGUMENT: the
// once-per-device shared-memory attribute (OSK_ENSURE_MAX_SMEM keeps its state in a function-local static) must be per kernel, and
// two instantiations of one kernel template have the same pointer type
template <void (*KERNEL)(const AttnParams)>
int launch_kernel(int smem_bytes, const AttnParams& p, hipStream_t st) {
  OSK_ENSURE_MAX_SMEM(KERNEL, smem_bytes);
  dim3 grid(attn_grid(p)), block(256);
  hipLaunchKernelGGL(KERNEL, grid, block, smem_bytes, st, p);
  return (int)hipGetLastError();
}

}  // namespace osk_attn
