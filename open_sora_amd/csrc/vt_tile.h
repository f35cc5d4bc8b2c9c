// The 64-key tile of V^T (include/osk.h, osk_v_transpose_bf16): the position -> key map of a head_dim and the store of one staged
// tile.  Shared by the kernels that write V^T from token-major V (elementwise.hip::v_transpose_kernel, kv_join.hip::kv_join_kernel),
// so the key order the attention kernels bake into their P operand is stated once.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// key (0..63, within its 64-key tile) stored at position pc * 8 + j of a V^T row; pc = the 16-byte chunk, j = the element in it
template <int HD>
__device__ __forceinline__ int vt_tile_key(int pc, int j) {
  if constexpr (HD == 72 || HD == 64) {
    // head_dim 72 and 64 (P.V on v_mfma_f32_16x16x32_bf16, attention_asm72.hip): chunk pc of the 64-key row = 32-key half pc / 4,
    // lane row r = pc % 4 of the MFMA operands, whose 8 keys are {0-3, 8-11}, {16-19, 24-27}, {4-7, 12-15}, {20-23, 28-31}
    const int r = pc & 3;
    return 32 * (pc >> 2) + ((r & 1) << 4) + ((r >> 1) << 2) + ((j >> 2) << 3) + (j & 3);
  } else {
    // head_dim 128 (P.V on 32x32x16): per 16 keys, positions 0-3 -> keys 0-3, 4-7 -> keys 8-11, 8-11 -> keys 4-7, 12-15 -> keys 12-15
    const int p = pc * 8 + j;                  // position within tile
    const int p16 = p & 15, grp = p & ~15;
    return grp + ((p16 < 4 || p16 >= 12) ? p16 : (p16 < 8 ? p16 + 4 : p16 - 4));
  }
}

// tile[key][d] (64 keys of one head, rows past the sequence end zero) -> HD rows of 64 positions at obase, rows Lp apart: 8 chunks of
// 8 keys per row, in the key order above; 256 threads, 16-byte stores
template <int HD>
__device__ __forceinline__ void vt_tile_store(const unsigned short (*tile)[HD + 2], unsigned short* obase, int Lp) {
  for (int i = threadIdx.x; i < HD * 8; i += 256) {
    const int d = i >> 3, pc = i & 7;  // pc: 8-position chunk within the 64-key row
    unsigned short e[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) e[j] = tile[vt_tile_key<HD>(pc, j)][d];
    uint4 u;
    u.x = e[0] | ((unsigned)e[1] << 16);
    u.y = e[2] | ((unsigned)e[3] << 16);
    u.z = e[4] | ((unsigned)e[5] << 16);
    u.w = e[6] | ((unsigned)e[7] << 16);
    *reinterpret_cast<uint4*>(obase + (int64_t)d * Lp + pc * 8) = u;
  }
}
