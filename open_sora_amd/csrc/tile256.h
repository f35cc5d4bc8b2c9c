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

// ---- Addressing rule of the 256-row tiles.  An LDS-DMA instruction adds a 32-bit UNSIGNED per-lane byte offset to a wave-uniform
// 64-bit base.  The base a kernel hands to its K loop is operand + the tile's ORIGIN -- the smallest element offset of the rows the
// tile's loaders touch -- and the lane offsets are relative to it: only the WINDOW of one tile (its 256 rows, a batch jump in the
// middle included, forwards or backwards) has to fit 32 bits, the operand may span any number of GiB.  The K axis advances the
// 64-bit base.  row_window() is that window, for the device (origin = lo) and for the host's support condition (windows_fit).
struct RowWindow { int64_t lo, hi; };   // smallest / largest element offset of the rows [first, last]

// rows first .. last (first <= last, both inside the operand) where row r lies at (r / rpb) * bs + min(r % rpb, valid - 1) * rs:
// batched rows whose positions behind `valid` read the last valid one (plain operands: rpb = valid = INT_MAX, bs = 0).  Inside a
// batch the offset is monotonic in the row, and whole batches between the first and the last one are linear in the batch index:
// the extremes are among the ends of the first, second, last-but-one and last batch's pieces.
static __host__ __device__ __forceinline__ RowWindow row_window(int first, int last, int rpb, int valid, int64_t bs, int64_t rs) {
  const int b0 = first / rpb, b1 = last / rpb;
  auto at = [&](int b, int l) { return b * bs + (int64_t)(l < valid ? l : valid - 1) * rs; };
  const int64_t x = at(b0, first - b0 * rpb), y = at(b0, b0 == b1 ? last - b1 * rpb : rpb - 1);
  RowWindow w{x < y ? x : y, x < y ? y : x};
  auto add = [&](int64_t v) { w.lo = v < w.lo ? v : w.lo; w.hi = v > w.hi ? v : w.hi; };
  if (b1 != b0) {
    add(at(b1, 0));
    add(at(b1, last - b1 * rpb));
    if (b1 - b0 > 1) {
      add(at(b0 + 1, 0)); add(at(b0 + 1, rpb - 1));
      add(at(b1 - 1, 0)); add(at(b1 - 1, rpb - 1));
    }
  }
  return w;
}
// the window of the tile whose first row is r0: rows r0 .. r0 + 255, those behind the operand's last row read that row
static __host__ __device__ __forceinline__ RowWindow tile_window(int r0, int rows, int rpb, int valid, int64_t bs, int64_t rs) {
  return row_window(r0, r0 + 255 < rows ? r0 + 255 : rows - 1, rpb, valid, bs, rs);
}

// host: does every 256-row window of an operand of `rows` rows (K elements of es bytes read per row) lie within 2^32 - 1 bytes
// of its own origin?  Forward strides and a whole operand inside 4 GiB: yes, without looking at the tiles.
inline bool windows_fit(int rows, int rpb, int valid, int64_t bs, int64_t rs, int K, int es) {
  constexpr int64_t LIMIT = 0xFFFFFFFFll;
  if (bs >= 0 && rs >= 0) {
    const int lmax = (rpb < rows ? rpb : rows) - 1;
    if (((rows - 1) / rpb * bs + (lmax < valid ? lmax : valid - 1) * rs + K) * es <= LIMIT) return true;
  }
  // one batch: every tile's window is the first one's, or a shorter one
  const int step = rpb >= rows ? rows : 256;
  for (int r0 = 0; r0 < rows; r0 += step) {
    const RowWindow w = tile_window(r0, rows, rpb, valid, bs, rs);
    if (w.hi - w.lo > (LIMIT / es) - K) return false;
  }
  return true;
}

}  // namespace osk_tile256
