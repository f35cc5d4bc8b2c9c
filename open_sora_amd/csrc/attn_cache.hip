// Attention broadcast of the sampler (I2VDenoiser.denoise(attn_broadcast=...)): the store and the load of a block's attention output
// between the workspace's v columns and the block's cache slot.  HBM-bound, 16 B per lane, no LDS, no arithmetic.
#include "osk_common.h"
#include "../../include/osk.h"

// =============================================================================================
// Row-mapped copy of bf16 [B, L, C] between two strided views, one of which is a cache of `cache_rows` batch rows:
//   to_cache != 0 (store):  dst[row_map[b], l, 0:C] = src[b, l, 0:C]
//   to_cache == 0 (load):   dst[b, l, 0:C]          = src[row_map[b], l, 0:C]
// row_map NULL = the identity.  The map lives on the device, so a captured graph replays it; a map entry outside [0, cache_rows) makes
// the kernel skip that batch item (nothing read, nothing written): a wrong map cannot reach memory outside the cache.
// Grid-stride over 16-byte chunks, at most 2048 workgroups of 256 lanes (8 per CU of the 256).  Bytes: 4 per element.
// =============================================================================================
__global__ void __launch_bounds__(256) attn_cache_copy_kernel(const unsigned short* __restrict__ src, int64_t sbs, int64_t srs,
                                                              unsigned short* __restrict__ dst, int64_t dbs, int64_t drs,
                                                              const int* __restrict__ row_map, int cache_rows, int to_cache,
                                                              unsigned L, unsigned C8, unsigned chunks) {
  const unsigned per_b = L * C8;              // chunks of one batch item (B L C / 8 < 2^31: checked by the entry point)
  for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < chunks; i += gridDim.x * 256u) {
    const unsigned b = i / per_b, r = i - b * per_b;
    const unsigned l = r / C8;
    const int64_t c = (int64_t)(r - l * C8) * 8;
    const int row = row_map ? row_map[b] : (int)b;
    if (row < 0 || row >= cache_rows) continue;
    const int64_t sb = to_cache ? (int64_t)b : (int64_t)row, db = to_cache ? (int64_t)row : (int64_t)b;
    *reinterpret_cast<uint4*>(dst + db * dbs + l * drs + c) = *reinterpret_cast<const uint4*>(src + sb * sbs + l * srs + c);
  }
}

extern "C" int osk_attn_cache_copy_bf16(const void* src, int64_t src_batch_stride, int64_t src_row_stride, void* dst,
                                        int64_t dst_batch_stride, int64_t dst_row_stride, const int32_t* row_map, int cache_rows,
                                        int to_cache, int B, int L, int C, void* stream) {
  if (!src || !dst || B <= 0 || L <= 0 || C <= 0 || (C & 7) || cache_rows <= 0) return OSK_EINVAL;
  if (!row_map && B > cache_rows) return OSK_EINVAL;
  if ((src_batch_stride & 7) || (src_row_stride & 7) || (dst_batch_stride & 7) || (dst_row_stride & 7)) return OSK_EINVAL;
  if (src_row_stride < C || dst_row_stride < C) return OSK_EINVAL;
  // the batch items of either side must not run into each other (the cache side has cache_rows of them, the other side B)
  const int src_items = to_cache ? B : cache_rows, dst_items = to_cache ? cache_rows : B;
  if (src_items > 1 && src_batch_stride < (int64_t)L * src_row_stride) return OSK_EINVAL;
  if (dst_items > 1 && dst_batch_stride < (int64_t)L * dst_row_stride) return OSK_EINVAL;
  if (((uintptr_t)src & 15) || ((uintptr_t)dst & 15) || ((uintptr_t)row_map & 3)) return OSK_EINVAL;
  const int64_t chunks = (int64_t)B * L * (C / 8);
  if (chunks >= (1ll << 31)) return OSK_EINVAL;
  int64_t nb = (chunks + 255) / 256;
  if (nb > 2048) nb = 2048;
  hipLaunchKernelGGL(attn_cache_copy_kernel, dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, (const unsigned short*)src,
                     src_batch_stride, src_row_stride, (unsigned short*)dst, dst_batch_stride, dst_row_stride, (const int*)row_map,
                     cache_rows, to_cache, (unsigned)L, (unsigned)(C / 8), (unsigned)chunks);
  return (int)hipGetLastError();
}
