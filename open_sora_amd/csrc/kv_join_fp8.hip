// The e4m3 counterparts of osk_kv_join_bf16 (kv_join.hip) for frame-window attention under sequence parallelism in fp8 mode:
//   osk_kv_quant_rows_fp8: a rank's bf16 rows [B, L, H*hd] -> token-major e4m3 bytes [B, L, H*hd] (its slot of a gather buffer), with
//     the arithmetic of attention_fwd.hip::k_pack_fp8_kernel / v_transpose_fp8_kernel: IEEE f32 division by the (batch, head) scale,
//     clamp to +-448, v_cvt_pk_fp8_f32.  Quantisation is element-wise, so the bytes are the ones those kernels produce for the same
//     element and scale -- only the layout differs, and that is the join's business.
//   osk_kv_join_fp8: the gathered, segment-major, token-major e4m3 V (and e4m3 or bf16 K) -> vt8 [B, H, vt8_rows(hd), round_up(L, 64)]
//     bit for bit as osk_v_transpose_fp8 writes it (key order of a 64-key tile, ones / validity row, zero rows) and K either as
//     k8 [B, H, round_up(L, 64), 128] bit for bit as osk_k_pack_fp8 writes it (rows L .. Lp-1 repeat row L-1) or, where K stays bf16
//     (pv8), the [B, L, H*hd] view osk_kv_join_bf16 writes.
// Both HBM-bound, one block = 64 keys x one head like the kernels they mirror; the join stages the V tile in LDS for the transposing
// store (rows of HD / 4 + 1 dwords: an odd stride, the byte gathers of a wave fall into distinct banks).
#include "osk_common.h"
#include "../../include/osk.h"

namespace {

OSK_DEV unsigned quant4(const float* f, float sc) {
  float g[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) g[e] = fminf(fmaxf(f[e] / sc, -448.0f), 448.0f);
  int r = 0;
  r = __builtin_amdgcn_cvt_pk_fp8_f32(g[0], g[1], r, false);
  r = __builtin_amdgcn_cvt_pk_fp8_f32(g[2], g[3], r, true);
  return (unsigned)r;
}

// x [B, L, H * HD] bf16 (strided) -> out [B, L, H * HD] e4m3 bytes (strided).  A thread converts 8-dim pieces (16 bytes in, 8 bytes
// out): a head of 72 bytes is no multiple of 16.  head_dim 128 takes two neighbouring pieces per thread and stores 16 bytes.
template <int HD>
__global__ void __launch_bounds__(256) kv_quant_rows_fp8_kernel(const unsigned short* __restrict__ x, int64_t bs, int64_t rs,
                                                                const float* __restrict__ scales, unsigned char* __restrict__ out,
                                                                int64_t obs, int64_t ors, int L, int H) {
  const int kt = blockIdx.x, h = blockIdx.y, b = blockIdx.z;
  const float sc = scales[b * H + h];
  constexpr int W = HD == 128 ? 16 : 8;      // dims per piece
  constexpr int PPR = HD / W;                // pieces per row
  for (int i = threadIdx.x; i < 64 * PPR; i += 256) {
    const int row = kt * 64 + i / PPR, c = i % PPR;
    if (row >= L) continue;
    const unsigned short* px = x + b * bs + (int64_t)row * rs + h * HD + c * W;
    unsigned char* po = out + b * obs + (int64_t)row * ors + h * HD + c * W;
    float f[W];
    unpack8(*reinterpret_cast<const uint4*>(px), f);
    if constexpr (W == 16) {
      unpack8(*reinterpret_cast<const uint4*>(px + 8), f + 8);
      *reinterpret_cast<uint4*>(po) = make_uint4(quant4(f, sc), quant4(f + 4, sc), quant4(f + 8, sc), quant4(f + 12, sc));
    } else {
      *reinterpret_cast<uint2*>(po) = make_uint2(quant4(f, sc), quant4(f + 4, sc));
    }
  }
}

// K8: K arrives as e4m3 segments and leaves as k8 (head_dim 128); else K arrives as bf16 segments and leaves as the bf16 view.
template <int HD, bool K8>
__global__ void __launch_bounds__(256) kv_join_fp8_kernel(const void* __restrict__ k_seg, int64_t kss, int64_t kbs, int64_t krs,
                                                          const unsigned char* __restrict__ v_seg, int64_t vss, int64_t vbs, int64_t vrs,
                                                          void* __restrict__ k_out, int64_t kobs, int64_t kors,
                                                          unsigned char* __restrict__ vt8, int seg_len, int L, int Lp, int H) {
  constexpr int RP = (HD + 1 + 15) / 16 * 16;
  constexpr int TS = HD / 4 + 1;             // dwords per tile row
  __shared__ unsigned tile[64][TS];
  const int kt = blockIdx.x, h = blockIdx.y, b = blockIdx.z;
  const int key0 = kt * 64;

  // ---- K
  if constexpr (K8) {
    static_assert(HD == 128, "k8 exists for head_dim 128");
    const unsigned char* ks = static_cast<const unsigned char*>(k_seg);
    unsigned char* k8 = static_cast<unsigned char*>(k_out);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int j = threadIdx.x + 256 * i;     // 64 rows x 8 pieces of 16 bytes
      const int row = key0 + (j >> 3), c = j & 7;
      const int src = row < L ? row : L - 1;   // rows L .. Lp-1 repeat row L-1
      const int s = src / seg_len;
      const uint4 u = *reinterpret_cast<const uint4*>(ks + s * kss + b * kbs + (int64_t)(src - s * seg_len) * krs + h * 128 + c * 16);
      *reinterpret_cast<uint4*>(k8 + ((int64_t)(b * H + h) * Lp + row) * 128 + c * 16) = u;
    }
  } else {
    const unsigned short* ks = static_cast<const unsigned short*>(k_seg);
    unsigned short* ko = static_cast<unsigned short*>(k_out);
    constexpr int CPR = HD / 8;
    for (int i = threadIdx.x; i < 64 * CPR; i += 256) {
      const int key = key0 + i / CPR, c = i % CPR;
      if (key >= L) continue;
      const int s = key / seg_len;
      const uint4 u = *reinterpret_cast<const uint4*>(ks + s * kss + b * kbs + (int64_t)(key - s * seg_len) * krs + h * HD + c * 8);
      *reinterpret_cast<uint4*>(ko + b * kobs + (int64_t)key * kors + h * HD + c * 8) = u;
    }
  }

  // ---- V: 64 keys x HD bytes into the tile (keys >= L: zero bytes = e4m3 +0, what the bf16 kernel quantises its zero rows to)
  constexpr int W = HD == 128 ? 16 : 8;        // bytes per piece
  constexpr int PPR = HD / W;
  for (int i = threadIdx.x; i < 64 * PPR; i += 256) {
    const int r = i / PPR, c = i % PPR;
    const int key = key0 + r;
    unsigned* dst = &tile[r][c * (W / 4)];
    if constexpr (W == 16) {
      uint4 u = make_uint4(0, 0, 0, 0);
      if (key < L) {
        const int s = key / seg_len;
        u = *reinterpret_cast<const uint4*>(v_seg + s * vss + b * vbs + (int64_t)(key - s * seg_len) * vrs + h * HD + c * W);
      }
      dst[0] = u.x; dst[1] = u.y; dst[2] = u.z; dst[3] = u.w;
    } else {
      uint2 u = make_uint2(0, 0);
      if (key < L) {
        const int s = key / seg_len;
        u = *reinterpret_cast<const uint2*>(v_seg + s * vss + b * vbs + (int64_t)(key - s * seg_len) * vrs + h * HD + c * W);
      }
      dst[0] = u.x; dst[1] = u.y;
    }
  }
  __syncthreads();
  // the store of v_transpose_fp8_kernel: thread = (row d, 16-byte chunk c of the 64-byte row); byte hi*32 + t2*16 + j*4 + e of the
  // tile row holds key 32 t2 + 8 j + 4 hi + e
  unsigned char* obase = vt8 + ((int64_t)(b * H + h) * RP) * Lp + key0;
  for (int i = threadIdx.x; i < RP * 4; i += 256) {
    const int d = i >> 2, c = i & 3;
    unsigned w[4];
#pragma unroll
    for (int q4 = 0; q4 < 4; ++q4) {
      const int pos = c * 16 + q4 * 4;
      const int hi = pos >> 5, s5 = pos & 31, t2 = s5 >> 4, j = (s5 & 15) >> 2;
      const int k0 = 32 * t2 + 8 * j + 4 * hi;
      unsigned r = 0;
      if (d < HD) {
#pragma unroll
        for (int e = 0; e < 4; ++e) r |= ((tile[k0 + e][d >> 2] >> (8 * (d & 3))) & 0xFFu) << (8 * e);
      } else if (d == HD) {
#pragma unroll
        for (int e = 0; e < 4; ++e) r |= (key0 + k0 + e < L ? 0x38u : 0u) << (8 * e);
      }
      w[q4] = r;
    }
    *reinterpret_cast<uint4*>(obase + (int64_t)d * Lp + c * 16) = make_uint4(w[0], w[1], w[2], w[3]);
  }
}

}  // namespace

extern "C" int osk_kv_quant_rows_fp8(const void* x, int64_t batch_stride, int64_t row_stride, const float* scales, void* out,
                                     int64_t o_batch_stride, int64_t o_row_stride, int B, int L, int H, int hd, void* stream) {
  if (!x || !scales || !out) return OSK_EINVAL;
  if (B <= 0 || B > 65535 || H <= 0 || H > 65535 || L <= 0) return OSK_EINVAL;
  // loads are 16 bytes of bf16; stores are 8 bytes (head_dim 72) or 16 bytes (head_dim 128) at multiples of the head width
  if (((uintptr_t)x & 15) || ((batch_stride | row_stride) & 7) || ((uintptr_t)scales & 3)) return OSK_EINVAL;
  if (((uintptr_t)out & 7) || ((o_batch_stride | o_row_stride) & 7)) return OSK_EINVAL;
  if (hd != 72 && hd != 128) return OSK_EUNSUPPORTED;
  if (hd == 128 && (((uintptr_t)out & 15) || ((o_batch_stride | o_row_stride) & 15))) return OSK_EINVAL;
  dim3 grid((L + 63) / 64, H, B), block(256);
  hipStream_t st = (hipStream_t)stream;
  if (hd == 72)
    hipLaunchKernelGGL(kv_quant_rows_fp8_kernel<72>, grid, block, 0, st, (const unsigned short*)x, batch_stride, row_stride, scales,
                       (unsigned char*)out, o_batch_stride, o_row_stride, L, H);
  else
    hipLaunchKernelGGL(kv_quant_rows_fp8_kernel<128>, grid, block, 0, st, (const unsigned short*)x, batch_stride, row_stride, scales,
                       (unsigned char*)out, o_batch_stride, o_row_stride, L, H);
  return (int)hipGetLastError();
}

extern "C" int osk_kv_join_fp8(const void* k_seg, int64_t k_seg_stride, int64_t k_batch_stride, int64_t k_row_stride, int k_kind,
                               const void* v_seg, int64_t v_seg_stride, int64_t v_batch_stride, int64_t v_row_stride, void* k_out,
                               int64_t ko_batch_stride, int64_t ko_row_stride, void* vt8_out, int B, int H, int hd, int n_seg,
                               int seg_len, int L, void* stream) {
  if (!k_seg || !v_seg || !k_out || !vt8_out) return OSK_EINVAL;
  if (k_kind != OSK_KV_JOIN_K_BF16 && k_kind != OSK_KV_JOIN_K_E4M3) return OSK_EINVAL;
  if ((((uintptr_t)k_seg | (uintptr_t)k_out | (uintptr_t)vt8_out) & 15) || ((uintptr_t)v_seg & 7)) return OSK_EINVAL;
  if (((v_seg_stride | v_batch_stride | v_row_stride) & 7)) return OSK_EINVAL;
  // K: 16-byte loads and stores -- 8 bf16 elements or 16 e4m3 bytes
  const int kmask = k_kind == OSK_KV_JOIN_K_E4M3 ? 15 : 7;
  if (((k_seg_stride | k_batch_stride | k_row_stride) & kmask)) return OSK_EINVAL;
  if (k_kind == OSK_KV_JOIN_K_BF16 && ((ko_batch_stride | ko_row_stride) & 7)) return OSK_EINVAL;
  if (B <= 0 || B > 65535 || H <= 0 || H > 65535 || n_seg <= 0 || seg_len <= 0 || L <= 0) return OSK_EINVAL;
  if ((int64_t)(n_seg - 1) * seg_len >= L || L > (int64_t)n_seg * seg_len) return OSK_EINVAL;
  if (hd != 72 && hd != 128) return OSK_EUNSUPPORTED;
  if (k_kind == OSK_KV_JOIN_K_E4M3 && hd != 128) return OSK_EUNSUPPORTED;
  if (hd == 128 && (((uintptr_t)v_seg & 15) || ((v_seg_stride | v_batch_stride | v_row_stride) & 15))) return OSK_EINVAL;
  const int Lp = (L + 63) / 64 * 64;
  dim3 grid(Lp / 64, H, B), block(256);
  hipStream_t st = (hipStream_t)stream;
#define LAUNCH(HD, K8)                                                                                                              \
  hipLaunchKernelGGL((kv_join_fp8_kernel<HD, K8>), grid, block, 0, st, k_seg, k_seg_stride, k_batch_stride, k_row_stride,         \
                     (const unsigned char*)v_seg, v_seg_stride, v_batch_stride, v_row_stride, k_out, ko_batch_stride,             \
                     ko_row_stride, (unsigned char*)vt8_out, seg_len, L, Lp, H)
  if (k_kind == OSK_KV_JOIN_K_E4M3) LAUNCH(128, true);
  else if (hd == 72) LAUNCH(72, false);
  else LAUNCH(128, false);
#undef LAUNCH
  return (int)hipGetLastError();
}
