// The 128 x 128 x 64 MFMA bf16 tile shared by the dense GEMM (gemm_bf16.hip) and the implicit-GEMM convolutions (conv3d.hip,
// conv2d.hip, dc_ae.hip):  acc[128 rows m][128 columns n] += A[m, k] * W[n, k]  over K tiles of 64.
//
// 256 threads = 4 waves (2 x 2), each wave 64 x 64 = 2 x 2 v_mfma_f32_32x32x16_bf16 tiles.  Operands are SWAPPED in the MFMA
// (A-operand = W fragment, B-operand = activation fragment) so that a lane of the accumulator owns one output ROW m and 4
// consecutive columns n per register quad: an epilogue is lane-local in m and stores 8 B (4 bf16) contiguous pieces.
//
// LDS layout.  Staging is HBM -> LDS with global_load_lds_dwordx4 (16 B per lane, LDS image lane-linear), double buffered, one
// barrier per K tile; a buffer is the A tile then the W tile, 128 rows of 128 B each.  A wave stages 4 row blocks of 8 rows per
// operand (1 KiB each: lane = row srow8, 16-byte position spos).  The 128-B rows are XOR-swizzled on the SOURCE side -- the lane
// that writes position spos of row r fetches source chunk spos ^ ((r >> 1) & 7) -- and un-swizzled on the ds_read_b128 side:
// conflict-free for the 32-row x 16-B fragment reads of the 32x32x16 MFMA.
//
// A user supplies what is its own: where the four 16-byte A chunks of a lane come from for K tile kt (a small by-value functor:
// by-reference captured arrays were placed in scratch by hipcc), and what happens to the accumulators.
#pragma once
#include "osk_common.h"

namespace osk_tile128 {

constexpr int BM = 128, BN = 128, BK = 64;
constexpr int TILE_BYTES = 128 * BK * 2;  // 16 KiB per operand tile
constexpr int SMEM_BYTES = 2 * 2 * TILE_BYTES;

OSK_DEV void glds16(const unsigned short* g, unsigned char* lds_wave_base) {
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)g,
                                   (__attribute__((address_space(3))) void*)lds_wave_base, 16, 0, 0);
}

// what a lane is in the tile: its workgroup's tile, its wave's quadrant, its 4 staging rows, its fragment read offsets
struct Lane {
  int bm, n0;                   // row band of the tile, first column of the tile
  int wm, wn, hi, l31;          // wave quadrant (2 x 2); half and row of the lane inside a 32 x 32 MFMA tile
  int row[4], cch[4];           // staging: tile row, and the source chunk that must land at LDS position spos
  int lds_off[4];               // byte offset of this wave's 1-KiB row block inside a tile (wave-uniform)
  const unsigned short* gw[4];  // W operand: row n0 + row[i] (clamped to the last row), chunk cch[i], K tile 0
  int a_row_off, w_row_off, sw; // fragment read offsets (bytes) inside a tile for ks = 0; other ks: chunk = (ks*2+hi) ^ sw
};

// M x N = the problem's rows x columns; w = [N][wrs] bf16
OSK_DEV Lane make_lane(int M, int N, const unsigned short* w, int64_t wrs) {
  Lane g;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  g.wm = wave >> 1, g.wn = wave & 1;
  g.hi = lane >> 5, g.l31 = lane & 31;

  const int nbm = (M + BM - 1) / BM, nbn = (N + BN - 1) / BN;
  const int tile = xcd_remap(blockIdx.x, nbm * nbn);
  g.bm = tile / nbn;
  g.n0 = (tile - g.bm * nbn) * BN;

  const int srow8 = lane >> 3, spos = lane & 7;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int rb = i * 4 + wave;
    const int r = rb * 8 + srow8;
    g.row[i] = r;
    g.cch[i] = spos ^ ((r >> 1) & 7);
    g.lds_off[i] = rb * 1024;
    int n = g.n0 + r;
    n = n < N ? n : N - 1;
    g.gw[i] = w + (int64_t)n * wrs + g.cch[i] * 8;
  }
  g.sw = (g.l31 >> 1) & 7;
  g.a_row_off = (g.wm * 64 + g.l31) * 128;
  g.w_row_off = (g.wn * 64 + g.l31) * 128;
  return g;
}

// tile row of this lane's accumulators acc[..][tm]
OSK_DEV int acc_row(const Lane& g, int tm) { return g.wm * 64 + tm * 32 + g.l31; }
// first of the 4 consecutive columns of registers qd * 4 .. qd * 4 + 3 of acc[tn][..]
OSK_DEV int acc_col(const Lane& g, int tn, int qd) { return g.n0 + g.wn * 64 + tn * 32 + qd * 8 + g.hi * 4; }

// one K tile (64) of the product, from the LDS images ta / tw
OSK_DEV void mma_ktile(const Lane& g, const unsigned char* ta, const unsigned char* tw, f32x16_t (&acc)[2][2]) {
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) {
    const int coff = (((ks << 1) | g.hi) ^ g.sw) << 4;
    bf16x8_t af[2], wf[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      af[t] = *reinterpret_cast<const bf16x8_t*>(ta + g.a_row_off + t * 32 * 128 + coff);
      wf[t] = *reinterpret_cast<const bf16x8_t*>(tw + g.w_row_off + t * 32 * 128 + coff);
    }
#pragma unroll
    for (int tn = 0; tn < 2; ++tn)
#pragma unroll
      for (int tm = 0; tm < 2; ++tm)
        acc[tn][tm] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf[tn], af[tm], acc[tn][tm], 0, 0, 0);
  }
}

// issue the 8 loads of K tile kt into buffer buf; a_src(g, i, kt) = global address of A chunk cch[i] of row row[i]
template <class ASrc>
OSK_DEV void stage_issue(const Lane& g, unsigned char* smem, int buf, int kt, const ASrc a_src) {
  unsigned char* ta = smem + buf * 2 * TILE_BYTES;
  unsigned char* tw = ta + TILE_BYTES;
#pragma unroll
  for (int i = 0; i < 4; ++i) glds16(a_src(g, i, kt), ta + g.lds_off[i]);
#pragma unroll
  for (int i = 0; i < 4; ++i) glds16(g.gw[i] + kt * BK, tw + g.lds_off[i]);
}

// acc = sum over nk K tiles: the double-buffered pipeline (issue next, multiply current, wait, barrier, flip)
template <class ASrc>
OSK_DEV void mainloop(const Lane& g, unsigned char* smem, int nk, const ASrc a_src, f32x16_t (&acc)[2][2]) {
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  stage_issue(g, smem, 0, 0, a_src);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  int cur = 0;
  for (int kt = 0; kt < nk; ++kt) {
    if (kt + 1 < nk) stage_issue(g, smem, cur ^ 1, kt + 1, a_src);
    const unsigned char* ta = smem + cur * 2 * TILE_BYTES;
    mma_ktile(g, ta, ta + TILE_BYTES, acc);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    cur ^= 1;
  }
}

// ---------------------------------------------------------------------------------------------------------------------------
// The convolutions: K runs tap-major / channel-minor (k = tap * Cin + ci, Cin = 8 << lg_cpt), so every 16-byte chunk of the A tile
// is 8 contiguous channels of ONE input pixel / voxel.

// tap and 8-channel chunk of A chunk cch of K tile kt.  BIGC: Cin % 64 == 0 -> a K tile lies inside one tap (tap is wave-uniform)
struct TapChunk { int tap, cc; };
template <bool BIGC>
OSK_DEV TapChunk tap_chunk(int kt, int cch, int lg_cpt) {
  const int cpt_mask = (1 << lg_cpt) - 1;
  if constexpr (BIGC) {
    const int q = kt * 8;
    return {q >> lg_cpt, (q & cpt_mask) + cch};
  } else {
    const int q = kt * 8 + cch;
    return {q >> lg_cpt, q & cpt_mask};
  }
}

// (dt, dh, dw) of tap of a k x k x k kernel, k = 1 or 3
struct Tap3 { int dt, dh, dw; };
OSK_DEV Tap3 tap3(int tap, int ks) {
  Tap3 t = {0, 0, 0};
  if (ks == 3) {
    t.dt = tap / 9;
    const int r = tap - t.dt * 9;
    t.dh = r / 3;
    t.dw = r - t.dh * 3;
  }
  return t;
}

// output index (row-major frame, ho, wo) of tile row r of row band bm.  brick: a tile is an 8 x 16 spatial brick of one frame of
// (Ho, Wo) (whole bricks: Ho % 8 == 0 and Wo % 16 == 0), so the 10 x 18 inputs its 3 x 3 taps read are shared by the whole tile
// through L1 / L2; otherwise the tiles walk the outputs row-major
OSK_DEV int tile_row_index(int brick, int bm, int r, int Ho, int Wo) {
  if (!brick) return bm * BM + r;
  const int bw = Wo >> 4, bh = Ho >> 3;
  const int bx = bm % bw;
  const int q = bm / bw;
  const int by = q % bh;
  const int frame = q / bh;
  return (frame * Ho + by * 8 + (r >> 4)) * Wo + bx * 16 + (r & 15);
}

// epilogue of this lane's output row acc[..][tm] at element offset roff:  out = [silu](acc + bias) + res, as bf16
OSK_DEV void conv_epilogue_row(const Lane& g, const f32x16_t (&acc)[2][2], int tm, int64_t roff, int Cout, const float* bias,
                               bool act, const unsigned short* res, unsigned short* out) {
  const bool vec_ok = (Cout & 3) == 0;
#pragma unroll
  for (int tn = 0; tn < 2; ++tn) {
#pragma unroll
    for (int qd = 0; qd < 4; ++qd) {
      const int n = acc_col(g, tn, qd);
      if (n >= Cout) continue;
      float v[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = acc[tn][tm][qd * 4 + j];
      if (vec_ok && n + 3 < Cout) {
        if (bias) {
          const float4 bv = *reinterpret_cast<const float4*>(bias + n);
          v[0] += bv.x; v[1] += bv.y; v[2] += bv.z; v[3] += bv.w;
        }
        if (act) {
#pragma unroll
          for (int j = 0; j < 4; ++j) v[j] = silu(v[j]);
        }
        if (res) {
          const uint2 rv = *reinterpret_cast<const uint2*>(res + roff + n);
          v[0] += bf16_lo(rv.x); v[1] += bf16_hi(rv.x); v[2] += bf16_lo(rv.y); v[3] += bf16_hi(rv.y);
        }
        uint2 o;
        o.x = pack_bf16x2(v[0], v[1]);
        o.y = pack_bf16x2(v[2], v[3]);
        *reinterpret_cast<uint2*>(out + roff + n) = o;
      } else {
        for (int j = 0; j < 4 && n + j < Cout; ++j) {
          float t = v[j] + (bias ? bias[n + j] : 0.f);
          if (act) t = silu(t);
          if (res) t += bf16_bits_to_f32(res[roff + n + j]);
          out[roff + n + j] = f32_to_bf16_bits(t);
        }
      }
    }
  }
}

// host: K layout of a convolution with ntaps taps of Cin = 8 * 2^j channels; the weight rows [Cout][w_row_stride] are zero-padded
// to a multiple of BK.  OSK_OK, or OSK_EINVAL for a row stride that does not hold the padded K
inline int conv_k_layout(int Cin, int ntaps, int64_t w_row_stride, int* lg_cpt, int* nk) {
  int lg = 0;
  while ((8 << lg) < Cin) ++lg;
  const int64_t K = (int64_t)ntaps * Cin;
  const int64_t Kp = (K + BK - 1) / BK * BK;
  if (w_row_stride < Kp || (w_row_stride & 7)) return OSK_EINVAL;
  *lg_cpt = lg;
  *nk = (int)(Kp / BK);
  return OSK_OK;
}

}  // namespace osk_tile128
