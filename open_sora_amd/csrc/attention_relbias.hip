// Self-attention with a learned relative-position bias (T5), gfx950.
//
// The reference's text encoder is Hugging Face's T5EncoderModel (opensora/models/text/conditioner.py:48-53: T5-v1.1-XXL over 512
// tokens, attention_mask=None).  T5 self-attention (T5Attention.forward) is non-causal, does NOT scale its scores and adds a
// per-head bias that depends on the relative distance j - i alone:
//   out[b, i, h, :] = sum_j softmax_j(scale * q[b,i,h,:] . k[b,j,h,:] + bias[h * bias_row_stride + (j - i) + (L - 1)]) * v[b,j,h,:]
// bias f32 [H, >= 2 L - 1]: the host expands the bucket embedding (32 buckets) into one row of 2 L - 1 distances per head, so no
// L x L score or bias matrix exists in HBM.
//
// Attention is ~2 % of the encoder's FLOPs: a compiler-scheduled kernel, not a generated asm loop.
//   * One workgroup (4 waves) per (batch, head, 64-query block); a wave owns 16 query rows, Q fragments stay in registers.
//   * 64-key tiles of K (key-major) and V^T (dim-major: a 2-byte scatter, V is read as stored) go through LDS; the next tile's
//     global loads are issued before the current tile's math.  Rows are LDS_STRIDE = 72 elements (144 bytes) apart: the 16-byte
//     reads of the 16 rows of an MFMA operand fall on distinct bank groups.
//   * The 127 bias entries a (64-query, 64-key) tile can touch -- distances k0 - q0 - 63 .. k0 - q0 + 63 -- are staged in LDS per
//     tile, already in log2 units; entries outside [0, 2 L - 2] (rows or keys past L) are read as 0, never from memory.
//   * S^T = K . Q^T and O^T = V^T . P^T on v_mfma_f32_16x16x32_bf16 (the layout of attention_short.hip): a lane owns ONE query
//     (lane % 16) and keys 4 (lane / 16) .. + 3 of every 16-key block, so the softmax statistics are two xor-shuffles away and the
//     packed probabilities of two key blocks ARE the B operand of the P.V product.
//   * Online softmax in f32; the bias is added before the running maximum (it is learned and unbounded: no bounded body).  Keys
//     >= L are masked with -inf before the maximum, their V rows are zero in LDS; query rows >= L are computed on a clamped row
//     and never stored.
//
// CAUSAL instantiation (osk_attention_causal_bf16: CLIP's text tower, conditioner.py:17-20, 48-53): no bias, out[b, i, h] sums over
// j <= i.  Query block qb walks the key tiles 0 .. qb only -- the tiles wholly above the diagonal are skipped, not masked -- and
// the diagonal tile (k0 == q0) masks j > i with -inf before the running maximum; key k0 <= i is visible to every row of every tile
// walked, so the maximum stays finite.  Staging, LDS layout and the MFMA layout are the ones above.
#include "../../include/osk.h"
#include "osk_common.h"

namespace {

struct RelBiasParams {
  const unsigned short* q; int64_t qbs, qrs;
  const unsigned short* k; int64_t kbs, krs;
  const unsigned short* v; int64_t vbs, vrs;
  unsigned short* out; int64_t obs, ors;
  const float* bias; int64_t brs;   // [H, >= 2 L - 1] or nullptr
  int B, H, L, nqb;                 // nqb = 64-query blocks per sequence
  float sc;                         // softmax scale * log2(e)
};

constexpr int RB_HD = 64;           // head dim
constexpr int RB_T = 64;            // query rows per workgroup == keys per tile
constexpr int LDS_STRIDE = 72;      // bf16 elements per LDS row (64 + 8)
constexpr float LOG2E = 1.4426950408889634f;

template <bool CAUSAL>
__global__ void __launch_bounds__(256) attn_relbias_kernel(const RelBiasParams p) {
  __shared__ __attribute__((aligned(16))) unsigned short ks[RB_T * LDS_STRIDE];    // K tile: row = key, 64 dims
  __shared__ __attribute__((aligned(16))) unsigned short vt[RB_HD * LDS_STRIDE];   // V^T tile: row = dim, 64 keys
  __shared__ float sb[128];                                                         // bias of distance index t = jl - il + 63
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l15 = lane & 15, g = lane >> 4;
  int unit = xcd_remap(blockIdx.x, gridDim.x);            // the query blocks of one (batch, head) share an XCD's L2
  const int qb = unit % p.nqb;
  unit /= p.nqb;
  const int h = unit % p.H, b = unit / p.H;
  const int L = p.L, q0 = qb * RB_T;
  const unsigned short* qg = p.q + b * p.qbs + h * RB_HD;
  const unsigned short* kg = p.k + b * p.kbs + h * RB_HD;
  const unsigned short* vg = p.v + b * p.vbs + h * RB_HD;
  const float* bg = p.bias ? p.bias + h * p.brs : nullptr;

  // ---- this lane's query: row il of the block (rows past the sequence: a duplicate of the last row, never stored)
  const int il = 16 * wave + l15;
  const bool qok = q0 + il < L;
  const int qi = qok ? q0 + il : L - 1;
  bf16x8_t qf[2];
#pragma unroll
  for (int s = 0; s < 2; ++s)
    qf[s] = __builtin_bit_cast(bf16x8_t, *reinterpret_cast<const uint4*>(qg + (int64_t)qi * p.qrs + (4 * s + g) * 8));

  // ---- staging: K chunk (key = i / 8, 16-byte chunk i % 8) for i = tid, tid + 256: coalesced rows;
  //      V chunk (key = tid % 64, chunk tid / 64 + 4 r): the 64 lanes of a wave scatter one dim row's 64 consecutive keys
  const int kkey0 = tid >> 3, kc = tid & 7;
  const int vkey = tid & 63, vc0 = tid >> 6;
  uint4 kr[2], vr[2];
  float br = 0.f;
  auto fetch = [&](int k0) {
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      const int kk = k0 + kkey0 + 32 * r, vk = k0 + vkey;
      kr[r] = kk < L ? *reinterpret_cast<const uint4*>(kg + (int64_t)kk * p.krs + kc * 8) : make_uint4(0, 0, 0, 0);
      vr[r] = vk < L ? *reinterpret_cast<const uint4*>(vg + (int64_t)vk * p.vrs + (vc0 + 4 * r) * 8) : make_uint4(0, 0, 0, 0);
    }
    if constexpr (!CAUSAL) {
      const int idx = k0 - q0 - (RB_T - 1) + (L - 1) + tid;             // distance index of sb[tid]
      br = (bg && tid < 2 * RB_T - 1 && idx >= 0 && idx <= 2 * L - 2) ? bg[idx] * LOG2E : 0.f;
    }
  };
  auto stage = [&]() {
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      *reinterpret_cast<uint4*>(ks + (kkey0 + 32 * r) * LDS_STRIDE + kc * 8) = kr[r];
      unsigned short* col = vt + ((vc0 + 4 * r) * 8) * LDS_STRIDE + vkey;
      const uint4 u = vr[r];
      col[0 * LDS_STRIDE] = (unsigned short)(u.x & 0xFFFF); col[1 * LDS_STRIDE] = (unsigned short)(u.x >> 16);
      col[2 * LDS_STRIDE] = (unsigned short)(u.y & 0xFFFF); col[3 * LDS_STRIDE] = (unsigned short)(u.y >> 16);
      col[4 * LDS_STRIDE] = (unsigned short)(u.z & 0xFFFF); col[5 * LDS_STRIDE] = (unsigned short)(u.z >> 16);
      col[6 * LDS_STRIDE] = (unsigned short)(u.w & 0xFFFF); col[7 * LDS_STRIDE] = (unsigned short)(u.w >> 16);
    }
    if constexpr (!CAUSAL)
      if (tid < 128) sb[tid] = br;
  };

  f32x4_t o[4];                     // O^T: dims 16 db + 4 g .. + 3 of query il
#pragma unroll
  for (int db = 0; db < 4; ++db) o[db] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  float m = -INFINITY, lsum = 0.f;  // running maximum (log2 units, whole row) and this lane's share of the denominator

  const int nkt = CAUSAL ? qb + 1 : (L + RB_T - 1) / RB_T;   // causal: the tiles above the diagonal are not walked
  fetch(0);
  for (int t = 0; t < nkt; ++t) {
    const int k0 = t * RB_T;
    __syncthreads();                // the previous tile's reads are done
    stage();
    __syncthreads();
    if (t + 1 < nkt) fetch(k0 + RB_T);
    // ---- scores (log2 units) of query il against keys k0 + 16 kb + 4 g + i
    f32x4_t s[4];
    float mt = -INFINITY;
#pragma unroll
    for (int kb = 0; kb < 4; ++kb) {
      s[kb] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        const uint4 a = *reinterpret_cast<const uint4*>(ks + (kb * 16 + l15) * LDS_STRIDE + (4 * c + g) * 8);
        s[kb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, a), qf[c], s[kb], 0, 0, 0);
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int jl = kb * 16 + 4 * g + i;
        float x;
        if constexpr (CAUSAL) {
          x = s[kb][i] * p.sc;
          x = (k0 + jl < L && k0 + jl <= q0 + il) ? x : -INFINITY;     // only the diagonal tile has j > i
        } else {
          x = __builtin_fmaf(s[kb][i], p.sc, sb[jl - il + (RB_T - 1)]);
          x = k0 + jl < L ? x : -INFINITY;
        }
        s[kb][i] = x;
        mt = fmaxf(mt, x);
      }
    }
    mt = fmaxf(mt, __shfl_xor(mt, 16, 64));
    mt = fmaxf(mt, __shfl_xor(mt, 32, 64));
    const float mn = fmaxf(m, mt);                         // finite: key k0 < L (causal: k0 <= q0 too) is in every tile
    const float alpha = __builtin_amdgcn_exp2f(m - mn);    // first tile: 2^(-inf) = 0
    m = mn;
    float psum = 0.f;
    unsigned pk[4][2];
#pragma unroll
    for (int kb = 0; kb < 4; ++kb) {
      float e[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        e[i] = __builtin_amdgcn_exp2f(s[kb][i] - mn);
        psum += e[i];
      }
      pk[kb][0] = pack_bf16x2(e[0], e[1]);
      pk[kb][1] = pack_bf16x2(e[2], e[3]);
    }
    lsum = lsum * alpha + psum;
    // ---- O^T block db += V^T rows (dim 16 db + l15; keys 32 kp + 4 g .. + 3 and 32 kp + 16 + 4 g .. + 3: the order the two score
    //      blocks hold them in) x the packed P of blocks 2 kp, 2 kp + 1
#pragma unroll
    for (int db = 0; db < 4; ++db) {
      o[db] *= alpha;
      const unsigned short* vrow = vt + (db * 16 + l15) * LDS_STRIDE + 4 * g;
#pragma unroll
      for (int kp = 0; kp < 2; ++kp) {
        const uint2 a0 = *reinterpret_cast<const uint2*>(vrow + 32 * kp), a1 = *reinterpret_cast<const uint2*>(vrow + 32 * kp + 16);
        const uint4 au = make_uint4(a0.x, a0.y, a1.x, a1.y), bu = make_uint4(pk[2 * kp][0], pk[2 * kp][1], pk[2 * kp + 1][0], pk[2 * kp + 1][1]);
        o[db] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, au), __builtin_bit_cast(bf16x8_t, bu), o[db], 0, 0, 0);
      }
    }
  }
  lsum += __shfl_xor(lsum, 16, 64);
  lsum += __shfl_xor(lsum, 32, 64);
  const float inv = 1.0f / lsum;
  if (qok) {
    unsigned short* orow = p.out + b * p.obs + (int64_t)qi * p.ors + h * RB_HD + 4 * g;
#pragma unroll
    for (int db = 0; db < 4; ++db) {
      uint2 w;
      w.x = pack_bf16x2(o[db][0] * inv, o[db][1] * inv);
      w.y = pack_bf16x2(o[db][2] * inv, o[db][3] * inv);
      *reinterpret_cast<uint2*>(orow + db * 16) = w;
    }
  }
}

}  // namespace

// argument checks shared by the two entry points + the launch of one instantiation
template <bool CAUSAL>
static int launch_relbias(const void* q, int64_t q_batch_stride, int64_t q_row_stride, const void* k, int64_t k_batch_stride,
                          int64_t k_row_stride, const void* v, int64_t v_batch_stride, int64_t v_row_stride, void* out,
                          int64_t o_batch_stride, int64_t o_row_stride, const float* bias, int64_t bias_row_stride, int B, int H, int L,
                          int hd, float scale, void* stream) {
  if (!q || !k || !v || !out || B <= 0 || H <= 0 || L <= 0) return OSK_EINVAL;
  if (hd != RB_HD || L > 4096) return OSK_EUNSUPPORTED;
  if ((q_batch_stride & 7) || (q_row_stride & 7) || (k_batch_stride & 7) || (k_row_stride & 7) || (v_batch_stride & 7) ||
      (v_row_stride & 7) || (o_batch_stride & 3) || (o_row_stride & 3))
    return OSK_EINVAL;
  if (((uintptr_t)q & 15) || ((uintptr_t)k & 15) || ((uintptr_t)v & 15) || ((uintptr_t)out & 7) || ((uintptr_t)bias & 3)) return OSK_EINVAL;
  if (bias && bias_row_stride < 2 * (int64_t)L - 1) return OSK_EINVAL;
  const int nqb = (L + RB_T - 1) / RB_T;
  const int64_t blocks = (int64_t)B * H * nqb;
  if (blocks > 0x7FFFFFFF) return OSK_EINVAL;
  RelBiasParams p{(const unsigned short*)q, q_batch_stride, q_row_stride, (const unsigned short*)k, k_batch_stride, k_row_stride,
                  (const unsigned short*)v, v_batch_stride, v_row_stride, (unsigned short*)out, o_batch_stride, o_row_stride,
                  bias, bias_row_stride, B, H, L, nqb, scale * LOG2E};
  hipLaunchKernelGGL(attn_relbias_kernel<CAUSAL>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, p);
  return (int)hipGetLastError();
}

extern "C" int osk_attention_relbias_bf16(const void* q, int64_t q_batch_stride, int64_t q_row_stride, const void* k,
                                          int64_t k_batch_stride, int64_t k_row_stride, const void* v, int64_t v_batch_stride,
                                          int64_t v_row_stride, void* out, int64_t o_batch_stride, int64_t o_row_stride,
                                          const float* bias, int64_t bias_row_stride, int B, int H, int L, int hd, float scale,
                                          void* stream) {
  return launch_relbias<false>(q, q_batch_stride, q_row_stride, k, k_batch_stride, k_row_stride, v, v_batch_stride, v_row_stride, out,
                               o_batch_stride, o_row_stride, bias, bias_row_stride, B, H, L, hd, scale, stream);
}

extern "C" int osk_attention_causal_bf16(const void* q, int64_t q_batch_stride, int64_t q_row_stride, const void* k,
                                         int64_t k_batch_stride, int64_t k_row_stride, const void* v, int64_t v_batch_stride,
                                         int64_t v_row_stride, void* out, int64_t o_batch_stride, int64_t o_row_stride, int B, int H,
                                         int L, int hd, float scale, void* stream) {
  return launch_relbias<true>(q, q_batch_stride, q_row_stride, k, k_batch_stride, k_row_stride, v, v_batch_stride, v_row_stride, out,
                              o_batch_stride, o_row_stride, nullptr, 0, B, H, L, hd, scale, stream);
}
