// osk_kv_join_bf16: the gathered, segment-major, token-major K and V of one block (the exchange buffers of sequence parallelism:
// key j in segment j / seg_len, row j % seg_len) -> the operands of ONE key segment of L keys: K as a [B, L, H*hd] view and V^T
// [B, H, hd, round_up(L, 64)] exactly as osk_v_transpose_bf16 writes it for a contiguous V.  HBM-bound: K and V are each read once and
// written once, 16 bytes per lane.  One block = 64 keys x one head, like elementwise.hip::v_transpose_kernel, whose LDS-staged tile
// store it shares (vt_tile.h); the only difference on the read side is the segment lookup of a key's row.
#include "osk_common.h"
#include "vt_tile.h"
#include "../../include/osk.h"

template <int HD>
__global__ void __launch_bounds__(256) kv_join_kernel(const unsigned short* __restrict__ k_seg, const unsigned short* __restrict__ v_seg,
                                                      int64_t ss, int64_t bs, int64_t rs, unsigned short* __restrict__ k_out,
                                                      int64_t kobs, int64_t kors, unsigned short* __restrict__ vt, int seg_len, int L,
                                                      int Lp, int H) {
  __shared__ unsigned short tile[64][HD + 2];  // +2: odd dword stride -> conflict-free column reads
  const int kt = blockIdx.x, h = blockIdx.y, b = blockIdx.z;
  const int key0 = kt * 64;
  constexpr int CPR = HD / 8;
  for (int i = threadIdx.x; i < 64 * CPR; i += 256) {
    const int r = i / CPR, c = i % CPR;
    const int key = key0 + r;
    uint4 u = make_uint4(0, 0, 0, 0);
    if (key < L) {   // (keys >= L: the padding rows of a short last segment are never read, V^T gets zeros, K has no such row)
      const int s = key / seg_len;
      const int64_t src = s * ss + b * bs + (int64_t)(key - s * seg_len) * rs + h * HD + c * 8;
      const uint4 kk = *reinterpret_cast<const uint4*>(k_seg + src);
      u = *reinterpret_cast<const uint4*>(v_seg + src);
      *reinterpret_cast<uint4*>(k_out + b * kobs + (int64_t)key * kors + h * HD + c * 8) = kk;
    }
    unsigned* dst = reinterpret_cast<unsigned*>(&tile[r][c * 8]);
    dst[0] = u.x; dst[1] = u.y; dst[2] = u.z; dst[3] = u.w;
  }
  __syncthreads();
  vt_tile_store<HD>(tile, vt + ((int64_t)(b * H + h) * HD) * Lp + key0, Lp);
}

extern "C" int osk_kv_join_bf16(const void* k_seg, const void* v_seg, int64_t seg_stride, int64_t batch_stride, int64_t row_stride,
                                void* k_out, int64_t ko_batch_stride, int64_t ko_row_stride, void* vt_out, int B, int H, int hd,
                                int n_seg, int seg_len, int L, void* stream) {
  if (!k_seg || !v_seg || !k_out || !vt_out) return OSK_EINVAL;
  if ((((uintptr_t)k_seg | (uintptr_t)v_seg | (uintptr_t)k_out | (uintptr_t)vt_out) & 15)) return OSK_EINVAL;
  if (((seg_stride | batch_stride | row_stride | ko_batch_stride | ko_row_stride) & 7)) return OSK_EINVAL;
  if (B <= 0 || B > 65535 || H <= 0 || H > 65535 || n_seg <= 0 || seg_len <= 0 || L <= 0) return OSK_EINVAL;
  if ((int64_t)(n_seg - 1) * seg_len >= L || L > (int64_t)n_seg * seg_len) return OSK_EINVAL;
  const int Lp = (L + 63) / 64 * 64;
  dim3 grid(Lp / 64, H, B), block(256);
  hipStream_t st = (hipStream_t)stream;
#define LAUNCH(HD)                                                                                                                    \
  hipLaunchKernelGGL(kv_join_kernel<HD>, grid, block, 0, st, (const unsigned short*)k_seg, (const unsigned short*)v_seg, seg_stride, \
                     batch_stride, row_stride, (unsigned short*)k_out, ko_batch_stride, ko_row_stride, (unsigned short*)vt_out,      \
                     seg_len, L, Lp, H)
  if (hd == 64) LAUNCH(64);
  else if (hd == 72) LAUNCH(72);
  else if (hd == 128) LAUNCH(128);
  else return OSK_EUNSUPPORTED;
#undef LAUNCH
  return (int)hipGetLastError();
}
