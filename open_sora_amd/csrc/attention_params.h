// Launch parameters shared by the flash-attention kernels (attention_fwd.hip, attention_asm{72,128}{,p8}.hip).
#pragma once
#include "osk_common.h"

namespace osk_attn {

struct AttnParams {
  const unsigned short* q;
  int64_t qbs, qrs;
  const unsigned short* k;
  int64_t kss, kbs, krs;
  const unsigned short* vt;
  int64_t vtss;
  unsigned short* out;
  int64_t obs, ors;
  float* lse;
  int B, H, Lq, n_seg, seg_len, seg_lp, tps;
  float sc;   // softmax scale * log2(e); 1.0 when q_prescaled
  // caller-supplied bound on the scores as the kernel sees them (|q . k| * sc <= bound, log2 units), rounded UP to a bf16 value;
  // 0 = unknown.  With a bound <= OSK_ATTN_MAX_BOUND the hand-scheduled kernels run their FAST body: reference max = bound (a
  // constant in Q's padding dim), no max tracking, branch-free loader advance; ragged segment-last tiles and segment jumps are
  // out-of-line events (tools/gen_attn_asm.py::fast_events).  Several segments of fewer than 3 tiles: the general body.
  float bound = 0.f;
  int q_prescaled;
  int rows = 256;   // query rows per work unit (workgroup): 256, or 512 for the wide head_dim-72 layout (attention_asm72w.hip)
  int Bkv;    // key / value batches: query batch b reads key batch b % Bkv
  int map;    // block -> (head, query block) order: 0 = heads fastest, 1 = XCD-contiguous, query blocks fastest
  // tail split (hand-scheduled kernels only; see split_tail()): the workgroups of the last, partial round of the grid
  // -- work units >= tail_first in launch order -- are cut into tail_split parts along the key axis; a part writes its
  // normalised partial O (f32) and its log2-domain LSE into the workspace and attn_merge_kernel combines them
  // INVARIANT: tail_first ALONE decides which epilogue a unit runs (block_to_work_split: unit >= tail_first writes f32 partials);
  // tail_split only says how many key parts such a unit has (attn_grid, key_part).  Every launch without partial results keeps
  // tail_first = 0x7fffffff -- split_tail() and the general twin of an auto-dispatched pair reset it -- and tail_first = 0 with
  // tail_split = 1 is the last-segment launch of osk_attention_fwd_ragged_bf16: every unit, one part, its whole key range.
  int tail_first = 0x7fffffff, tail_split = 1;
  float* ws_o = nullptr;
  float* ws_lse = nullptr;
  // fp8 P.V variant (attention_asm*p8.hip): V^T as e4m3 [Bkv, H, RP, seg_lp] per segment (vtss in BYTES) from
  // osk_v_transpose_fp8, one f32 scale per (key batch, head)
  const unsigned char* vt8 = nullptr;
  const float* v_scale = nullptr;
  // fp8 QK^T variant (attention_asm128q8.hip): K as e4m3 [Bkv, H, seg_lp, 128] per segment from osk_k_pack_fp8 (kss, kbs in BYTES,
  // krs = 128), one f32 scale per (key batch, head)
  const unsigned char* k8 = nullptr;
  const float* k_scale = nullptr;
  // device-derived score bound (round 6, osk_attention_fwd_auto_bf16): squared row-norm maxima of the q and k the kernel receives,
  // per (batch, head) -- qn2 [B, H], kn2 [Bkv, H], from osk_rownorm2_max_bf16.  With both set, every workgroup derives ITS bound
  // sqrt(qn2 kn2) (Cauchy-Schwarz on the actual operands) and the launch is one of a PAIR over the same grid: the FAST kernel's
  // workgroups run where that bound is <= OSK_ATTN_MAX_BOUND and exit at once elsewhere, the general kernel's the other way round
  // (attn_auto_bound below) -- no host round trip, no promise from the caller, hipGraph-capturable.
  const float* qn2 = nullptr;
  const float* kn2 = nullptr;
  // per query block key window (osk_attention_fwd_window_bf16): device table [ceil(Lq / 256)][2] of (first tile, tile count), in
  // 64-key tiles of the launch's single segment; query block qb visits tiles [first, first + count) only (key_part() below).  Only
  // launches of 256-row units with n_seg == 1 that write finished rows carry one: no wide layout, no tail split.
  const int* win = nullptr;
};

#define OSK_ATTN_MAX_BOUND 56.0f   // P = exp2(s - bound) >= 2^-112 for every admissible score: no underflow to zero

static inline bool attn_fast_path(const AttnParams& p) {   // host side
  return p.bound > 0.f && p.bound <= OSK_ATTN_MAX_BOUND && (p.n_seg == 1 || p.tps >= 3);
}

// Which of the two kernels of an auto-dispatched pair works on (batch b, head h), and with which bound?  Host-decided launches
// (qn2 == nullptr): every workgroup runs, bound = the caller's.  Returns false when THIS kernel (fast_kernel: its FAST instantiation)
// must leave the unit to its twin.  Wave-uniform (scalar loads).
OSK_DEV bool attn_auto_bound(const AttnParams& p, int b, int h, bool fast_kernel, float& bound) {
  bound = p.bound;
  if (!p.qn2) return true;
  // the norms are those of the bf16 values the MFMA multiplies: |q . k| <= |q| |k| exactly; 1.004 covers the f32 rounding of the
  // products and the square root; then UP to the next bf16 value (the kernels keep the bound in a bf16 field of Q's padding dim)
  const float v = __builtin_sqrtf(p.qn2[b * p.H + h] * p.kn2[(b % p.Bkv) * p.H + h]) * 1.004f;
  bound = __uint_as_float((__float_as_uint(v) + 0xFFFFu) & 0xFFFF0000u);
  const bool fast_ok = bound <= OSK_ATTN_MAX_BOUND;      // (NaN / inf norms: false -> the general body)
  return fast_ok == fast_kernel;
}

// (batch*head, query block) of a workgroup.  map 1 hands every XCD (block b runs on XCD b % 8) a contiguous
// range of the (head-major) work list, so the workgroups resident on one XCD walk the SAME head's K / V^T
// stream together and share it through that XCD's private L2.
OSK_DEV void block_to_work(const AttnParams& p, int nqb, int& bh, int& qb) {
  const int nbh = p.B * p.H;
  if (p.map == 1) {
    const int w = xcd_remap(blockIdx.x, nqb * nbh);
    bh = w / nqb;
    qb = w - bh * nqb;
  } else {
    bh = blockIdx.x % nbh;
    qb = blockIdx.x / nbh;
  }
}

// work unit index (launch order) -> (batch*head, query block)
OSK_DEV void unit_to_work(const AttnParams& p, int nqb, int unit, int& bh, int& qb) {
  const int nbh = p.B * p.H;
  if (p.map == 1) {
    const int w = xcd_remap(unit, nqb * nbh);
    bh = w / nqb;
    qb = w - bh * nqb;
  } else {
    bh = unit % nbh;
    qb = unit / nbh;
  }
}

// block -> work unit (+ key part of a split tail unit).  Returns true for a part of a split unit; tail_unit = its index
// among the tail units (workspace slot).
OSK_DEV bool block_to_work_split(const AttnParams& p, int nqb, int& bh, int& qb, int& part, int& tail_unit) {
  int unit = blockIdx.x;
  part = 0;
  tail_unit = 0;
  // (tail_first is 0x7fffffff in every launch without partial results; tail_split == 1 with tail_first == 0 is the last-segment launch of
  //  osk_attention_fwd_ragged_bf16: every unit writes its f32 partial over its whole key range)
  const bool tail = unit >= p.tail_first;
  if (tail) {
    const int j = unit - p.tail_first;
    tail_unit = j / p.tail_split;
    part = j - tail_unit * p.tail_split;
    unit = p.tail_first + tail_unit;
  }
  unit_to_work(p, nqb, unit, bh, qb);
  return tail;
}

// key range of a part: element offsets of its first tile into K and V^T, its tile counts, whether it ends in the ragged tile
struct KeyPart {
  int64_t k_off, v_off;
  int tps, nt;
  bool ragged;
};
OSK_DEV KeyPart key_part(const AttnParams& p, bool tail, int part, int qb, bool ragged) {
  KeyPart r{0, 0, p.tps, p.n_seg * p.tps, ragged};
  if (tail) {
    if (p.n_seg > 1) {   // whole key segments per part (tail_split divides n_seg)
      const int per = p.n_seg / p.tail_split;
      r.k_off = (int64_t)part * per * p.kss;
      r.v_off = (int64_t)part * per * p.vtss;
      r.nt = per * p.tps;
    } else {             // a run of tiles of the single segment; only the last part ends in the (possibly ragged) last tile
      const int t0 = part * p.tps / p.tail_split, t1 = (part + 1) * p.tps / p.tail_split;
      r.k_off = (int64_t)t0 * 64 * p.krs;
      r.v_off = (int64_t)t0 * 64;
      r.tps = r.nt = t1 - t0;
      r.ragged = ragged && part == p.tail_split - 1;
    }
  } else if (p.win && p.n_seg == 1) {
    // the query block's window: a run of tiles of the single segment, in the form the single-segment tail branch above hands the
    // loaders -- offsets of its first tile, tps = nt = its length (so the loaders never take a segment jump), ragged only where it
    // ends in the segment's last tile.  Runs of 1 and 2 tiles are nothing new to the loops: split tail parts of one tile, full and
    // ragged, run in both bodies (tests/attention_cases.py: f72_one_tile_per_part, g128_3tiles_plain_merge128), and a 2-tile run
    // is what a whole 128-key call is (tps = nt = 2).  k_loader / vt_loader take only the offsets (their segment jump is never
    // taken with tps == nt), lds_mask_first_tile covers the 1-tile ragged run, and loader_slots* see only `ragged`.  qb is
    // wave-uniform, so the two reads are scalar loads.  The table is clamped here: whatever it holds, the run stays inside the
    // segment.
    int t0 = p.win[2 * qb], n = p.win[2 * qb + 1];
    t0 = t0 < 0 ? 0 : (t0 > p.tps - 1 ? p.tps - 1 : t0);
    n = n < 1 ? 1 : (n > p.tps - t0 ? p.tps - t0 : n);
    r.k_off = (int64_t)t0 * 64 * p.krs;
    r.v_off = (int64_t)t0 * 64;
    r.tps = r.nt = n;
    r.ragged = ragged && t0 + n == p.tps;
  }
  return r;
}

// host: work units (workgroups before the tail split) of a launch, and its grid: every split tail unit takes tail_split workgroups.
// p.rows is the geometry of the kernel that is launched: the entry points pick the kernel from it (attention_fwd.hip)
static inline int attn_units(const AttnParams& p) { return ((p.Lq + p.rows - 1) / p.rows) * p.B * p.H; }
static inline int attn_grid(const AttnParams& p) {
  const int units = attn_units(p);
  return p.tail_split > 1 ? units + (units - p.tail_first) * (p.tail_split - 1) : units;
}

// host: decide the tail split of a launch of `units` work units given the workspace (attention_fwd.hip)
void split_tail(AttnParams& p, int units, int hd, void* workspace, int64_t workspace_bytes);
int launch_merge(const AttnParams& p, int hd, hipStream_t st);
// attention_merge.hip: fold the f32 partials (p.ws_o, p.ws_lse x lse_b_mult = natural log) of a launch whose every unit wrote one
// (tail_first == 0, tail_split == 1) into the finished rows p.out / p.lse of another launch over other keys, in place.
// unit_order: p.map's (the launch order of the attention kernels), or OSK_ATTN_ORDER_PLAIN = unit (b * H + h) * nqb + qb
#define OSK_ATTN_ORDER_PLAIN 2
int launch_merge_into(const AttnParams& p, int hd, float lse_b_mult, hipStream_t st);
// (the same with a second partial in one pass: launch_merge_into2 of attention_merge_into2.h)

// attention_asm72.hip: head_dim 72, 4 waves x 64 query rows, hand-scheduled (generated) main loop
int launch_asm72(const AttnParams& p, hipStream_t st);
// attention_asm72w.hip: head_dim 72, the bounded body in the wide layout (4 waves x 128 rows, one 32-key half per loop body); p.rows == 512
int launch_asm72w(const AttnParams& p, hipStream_t st);
// host: does a bounded head_dim-72 call take the wide layout?  (enough query rows for 512-row work units to fill the chip evenly)
// the same two kernels on tensors with 64-wide heads (template parameter HD = 64)
int launch_asm64(const AttnParams& p, hipStream_t st);
int launch_asm64w(const AttnParams& p, hipStream_t st);
// Rounds of the chip a launch of `units` equal work units takes, in units of one work unit's time: whole rounds plus the last,
// partial one -- which costs a full round without a workspace and min over the admissible key splits s of ceil(R s / CUs) / s with
// one (split_tail below makes the same choice).
static inline double attn_launch_rounds(const AttnParams& p, int units, int cus, bool has_ws) {
  const int R = units % cus;
  double tail = R ? 1.0 : 0.0;
  if (R && has_ws)
    for (int s = 2; s <= 8; ++s) {
      if (p.n_seg > 1 ? (p.n_seg % s != 0) : (s > p.tps)) continue;
      const double c = (double)((R * s + cus - 1) / cus) / s;
      if (c < tail) tail = c;
    }
  return (double)(units / cus) + tail;
}
// 512-row (wide) or 256-row work units for a bounded head_dim 72 / 64 call?  By estimated time, as tile_choice() does for the
// GEMMs (round 4 looked at Lq >= 1024 only: with few batch x head pairs -- B = 1, or a head-parallel sequence-parallel rank with
// H / P heads -- halving the unit count can leave most of the chip idle): a wide unit does the work of two narrow ones
// in 1.85 x the time (-7.4 % per launch measured where both fill the chip, profiles/r04e_attn_wide_step_ab.jsonl).
static inline bool attn_wide_path(const AttnParams& p, int hd, int cus, bool has_ws) {
#ifdef OSK_ATTN_NO_WIDE   // (A/B builds of tools/make_attn_nowide_lib.sh: always the 256-row layout)
  (void)p; (void)hd; (void)cus; (void)has_ws;
  return false;
#else
  if (!((hd == 72 || hd == 64) && attn_fast_path(p) && p.Lq >= 1024) || p.win) return false;   // (a window table is per 256 rows)
  const int bh = p.B * p.H;
  const double narrow = attn_launch_rounds(p, ((p.Lq + 255) / 256) * bh, cus, has_ws);
  const double wide = 1.852 * attn_launch_rounds(p, ((p.Lq + 511) / 512) * bh, cus, has_ws);
  return wide <= narrow;
#endif
}
// attention_asm128.hip: head_dim 128, the same layout and generator
int launch_asm128(const AttnParams& p, hipStream_t st);
// attention_asm128p8.hip / attention_asm72p8.hip: the same with the P.V product on the fp8 MFMA
int launch_asm128p8(const AttnParams& p, hipStream_t st);
int launch_asm72p8(const AttnParams& p, hipStream_t st);
// attention_asm128q8.hip: head_dim 128 with QK^T on the fp8 MFMA as well (K e4m3 from osk_k_pack_fp8, Q quantised in the prologue)
int launch_asm128q8(const AttnParams& p, hipStream_t st);

}  // namespace osk_attn
