// The frame around the 256-row tiles: what gemm256.hip, gemm256p.hip, gemm256x.hip and conv3d_256.hip do the same way OUTSIDE their
// generated K loops -- the order the tiles are walked in, the size of a persistent grid, and which source row and 16-byte chunk a lane
// of an LDS-DMA instruction fetches.  (The K loops are tools/gen_gemm_asm.py's and tools/gen_conv_sw_asm.py's; the epilogues are
// gemm_epilogue.h / gemm_epilogue16.h.)
#pragma once
#include "gemm_params.h"

namespace osk_tile256 {

// Tile order inside one problem of nbm x nbn tiles.  Every XCD (private 4 MiB L2) owns a contiguous range of the list (xcd_remap, by
// the caller); inside it the tiles run in groups of grp row bands, N-major within a group: the ~32 tiles resident on an XCD cover grp
// bands x a few weight tiles, so a weight tile is streamed once per grp bands instead of once per ~2 (OSK_GEMM_GROUP, default 8).
struct TileBlock { int bm, bn; };
OSK_DEV TileBlock grouped_tile(int tile, int nbm, int nbn, int grp) {
  const int per_group = grp * nbn;
  const int g = tile / per_group, r = tile - g * per_group;
  const int rows_here = nbm - g * grp < grp ? nbm - g * grp : grp;   // last group may be short
  const int bn = r / rows_here;
  return {g * grp + (r - bn * rows_here), bn};
}

// host: one workgroup per CU.  A persistent tile walk (tile i, i + grid, ...) keeps a workgroup inside one XCD's range of the list
// only for a grid that is a multiple of 8.
inline int persistent_grid(int ntiles) {
  int n_cu = osk_device_cus();
  n_cu -= n_cu % 8;
  if (n_cu < 8) n_cu = 8;
  return ntiles < n_cu ? ntiles : n_cu;
}

// LDS-DMA sources.  A stage is 128-byte rows; instruction j = wave + WAVES * i of a wave covers tile rows [8 j, 8 j + 8): lane l
// writes 16-byte position l % 8 of row 8 j + l / 8.  The rows are XOR-swizzled on the SOURCE side -- the lane that writes position
// l % 8 of row r fetches source chunk (l % 8) ^ ((r >> 1) & 7) -- and un-swizzled by the fragment reads.
template <int WAVES>
OSK_DEV int dma_row(int wave, int lane, int i) { return (wave + WAVES * i) * 8 + (lane >> 3); }
OSK_DEV int dma_chunk(int lane, int row) { return (lane & 7) ^ ((row >> 1) & 7); }

// element offset of row m of a batched A operand (rows behind M read row M - 1: finite values, dropped by the epilogue)
OSK_DEV int64_t a_row_offset(const osk_gemm::GemmParams& p, int m) {
  m = m < p.M ? m : p.M - 1;
  const int b = m / p.arpb, l = m - b * p.arpb;
  return b * p.abs_ + (int64_t)l * p.ars;
}
// element offset of row n of a plain W operand (rows behind N read row N - 1)
OSK_DEV int64_t w_row_offset(const osk_gemm::GemmParams& p, int n) {
  n = n < p.N ? n : p.N - 1;
  return (int64_t)n * p.wrs;
}

}  // namespace osk_tile256
