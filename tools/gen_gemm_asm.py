#!/usr/bin/env python
"""Generator of the hand-scheduled gfx950 K loops of the large-tile kernels: the persistent bf16 GEMMs (csrc/gemm256x.hip,
csrc/gemm256p.hip), the fp8 GEMM (csrc/gemm256.hip) and the implicit-GEMM CausalConv3d (csrc/conv3d_256.hip).

All four share one LDS image: two stages of [256][64] activations + [BN][64] weights, 128-byte rows, source-side XOR swizzle,
filled by LDS-DMA (global_load_lds_dwordx4, 1 KiB per wave instruction); operands swapped as in gemm_bf16.hip (A operand = weight
fragment, B operand = activation fragment: a lane of the accumulator owns one output row m); accumulators in AGPRs a[0 : NACC), which
the wrapper reads out for the fused epilogue.  Two wave layouts read it:
  Cfg    8 waves = 512 threads (two per SIMD) in a WM x WN grid, each wave TM x TN v_mfma_f32_32x32x16_bf16 tiles
           BN = 256: waves 2 x 4, wave tile 128 x 64  (TM 4, TN 2, 128 accumulator AGPRs)
           BN = 128: waves 4 x 2, wave tile  64 x 64  (TM 2, TN 2,  64 accumulator AGPRs)
         gen_pers (bf16, BN = 128) and gen_fp8 (one v_mfma_f32_32x32x64_f8f6f4 per two bf16 k-sub-steps)
  Cfg4x  4 waves (one per SIMD, the whole 512-register file each), wave tile 128 x 16 NBJ on v_mfma_f32_16x16x32_bf16
         gen_x4 and gen_conv_x4
One K step of a wave (after the barrier that published stage `cur`): the LAST k-sub-step of the previous K step (fragments
already in registers) with the LDS-DMA of stage cur^1 in its shadows | the other k-sub-steps, each prefetching the fragments
of the next into the other fragment set | vmcnt(0) lgkmcnt(0), barrier.

Every building block below is a plain function that returns (or emits) a list of instruction strings and exists once; a gen_*
function is the order in which one kernel issues them.
"""
import argparse
import os

from asm_emit import ar, clobbers, header, vr, write_body

SCRIPT = "gen_gemm_asm.py"

# asm-owned scalars.  Every loop: A / W running pointers (pairs), K steps, LDS destinations, K step done / fetched, temporaries
S_AB, S_WB, S_NK, S_ADST, S_WDST, S_T, S_KL, S_TMP, S_STEP = 40, 42, 44, 45, 46, 47, 48, 49, 50
S_PFLAGS, S_PBIAS = 52, 54                          # persistent GEMMs: flags; bias base (pair)
S_NKT, S_SIT, S_TAPOFF, S_XB2 = 52, 53, 54, 56      # conv: K steps per tap, step inside the tap, tap * 1024, x base (pair)
S_FIRST, S_LAST = 40, 51
# last scalar of each wrapper's clobber list (the 4-wave GEMM's list reaches past the registers its loop names: kept as generated)
PERS_S_LAST, W4_S_LAST, CONV_S_LAST = 55, 72, 57
PF_PREFETCHED, PF_HAS_NEXT, PF_BIAS = 0, 1, 2       # flag bits of the persistent GEMMs


def operand_table(names):
    return {n: "%%%d" % i for i, n in enumerate(names)}


# inline-asm operands of the four wrappers: fp8 GEMM, 8-wave persistent GEMM, 4-wave persistent GEMM, 4-wave conv
OP = operand_table(["faA0", "faA1", "faA2", "faA3", "faW0", "faW1", "faW2", "faW3", "aoff0", "aoff1", "aoff2", "aoff3",
                    "woff0", "woff1", "woff2", "woff3", "abase", "wbase", "nk", "adst", "wdst"])
POP = operand_table(["faA0", "faW0", "aoff0", "aoff1", "aoff2", "aoff3", "woff0", "woff1", "woff2", "woff3",
                     "aoffn0", "aoffn1", "aoffn2", "aoffn3", "woffn0", "woffn1", "woffn2", "woffn3", "boff",
                     "abase", "wbase", "bias", "nk", "adst", "wdst", "flags", "abasen", "wbasen"])
WOP = operand_table(["faA0", "faW0"] + ["aoff%d" % i for i in range(8)] + ["woff%d" % i for i in range(8)] +
                    ["boff", "abase", "wbase", "bias", "nk", "adst", "wdst", "flags", "abasen", "wbasen", "aoffp", "woffp"])
CWOP = operand_table(["faA0", "faW0", "arow0", "chk"] + ["woff%d" % i for i in range(8)] + ["xbase", "wbase", "nk", "nkt", "adst", "wdst"])


class Cfg:
    """8 waves on 32 x 32 MFMA tiles (see the module docstring); fp8: the same tile with K = 128 per step"""

    def __init__(self, bn, fp8=False):
        self.BN = bn
        self.FP8 = fp8
        self.TM, self.TN = (4, 2) if bn == 256 else (2, 2)
        self.TILE = 32                           # rows = columns of an MFMA tile
        self.NFA, self.NFW = self.TM, self.TN    # activation / weight fragments per k-sub-step, FSTRIDE LDS bytes (TILE rows) apart
        self.FSTRIDE = 128 * self.TILE
        self.NSUB = 4                            # k-sub-steps (ds_read_b128 columns of 32 bytes) per K step
        self.ACCW = 16                           # accumulator registers per MFMA tile
        self.MFMA = "v_mfma_f32_32x32x64_f8f6f4" if fp8 else "v_mfma_f32_32x32x16_bf16"
        self.NA, self.NW = 4, bn // 64           # LDS-DMA instructions per wave and stage (A: 32 / 8, W: BN/8 / 8)
        self.DMA_STRIDE = 8192                   # LDS bytes between a wave's consecutive LDS-DMA instructions (8 waves x 1 KiB)
        self.A_STAGE, self.W_STAGE = 32768, bn * 128
        self.W_BASE = 65536
        self.SMEM = self.W_BASE + 2 * self.W_STAGE
        self.NACC = 16 * self.TM * self.TN
        self.NFRAG = self.TM + self.TN
        # first asm-owned VGPR: two fragment sets.  fp8: a fragment is 32 bytes (8 registers), and with 128
        # accumulator AGPRs of the 256 registers a wave may own (two waves per SIMD) the VGPR half ends at v127
        self.FW = 8 if fp8 else 4
        self.V0 = (32 if bn == 256 else 64) if fp8 else 64
        self.VN = 2 * self.NFRAG * self.FW
        self.tag = ("q%d" if fp8 else "g%d") % bn

    def frag(self, fset, idx):                   # idx: 0..NFA-1 activation fragments, NFA.. weight fragments
        return self.V0 + (fset * self.NFRAG + idx) * self.FW


class Cfg4x:
    """4 waves x (128 x 128) on v_mfma_f32_16x16x32_bf16: 8 x 8 accumulator tiles of 16 x 16 (4 registers each, 256 AGPRs),
    a K step = TWO sub-steps of K = 32.  A fragment is 16 rows x 32 k -- one ds_read_b128 per lane (row
    l % 16, k group l / 16) out of the SAME LDS image (rows of 128 bytes, 16-byte chunk c of row r at (c ^ ((r >> 1) & 7))):
    conflict-free for this lane map too.  A sub-step reads 16 fragments for 64 MFMAs: less LDS read traffic per flop than the
    8-wave layouts and half the waves per barrier.  Why 16x16x32 (profiles/r02_gemm_experiments.md): with the K loop otherwise
    unchanged, issuing the same flops as 16x16x32 instead of 32x32x16 MFMAs is worth +5-7 % at the board's power cap (4
    accumulator registers written per 16 matrix cycles instead of 16 per 32)."""

    def __init__(self, nbj=8):
        self.NB = 8                             # 16-row blocks per wave tile (128 rows)
        self.NBJ = nbj                          # 16-column blocks per wave tile: 8 (256-wide workgroup tile) or 4 (128-wide)
        self.BN = 32 * nbj
        self.TILE = 16
        self.NFA, self.NFW = self.NB, nbj       # activation / weight fragments per sub-step, FSTRIDE LDS bytes (TILE rows) apart
        self.FSTRIDE = 128 * self.TILE
        self.NSUB = 2
        self.ACCW = 4
        self.MFMA = "v_mfma_f32_16x16x32_bf16"
        self.NA, self.NW = 8, nbj               # LDS-DMA instructions per wave and stage (32 KiB / 4 waves / 1 KiB)
        self.DMA_STRIDE = 4096                  # LDS bytes between a wave's consecutive LDS-DMA instructions (4 waves x 1 KiB)
        self.A_STAGE, self.W_STAGE = 32768, 4096 * nbj
        self.W_BASE = 65536
        self.SMEM = self.W_BASE + 2 * self.W_STAGE
        self.NACC = 32 * nbj
        self.NFRAG = 8 + nbj                    # activation + weight fragments per sub-step
        self.FW = 4
        self.V0 = 96                            # asm-owned VGPRs: v96.. (two fragment sets, then the address registers)
        self.VN = 2 * self.NFRAG * self.FW
        self.tag = "x%d" % self.BN

    def frag(self, fset, idx):
        return self.V0 + (fset * self.NFRAG + idx) * self.FW


class Emit:
    """the lines of one asm statement; label names end in %= (unique per emitted copy of the statement)"""

    def __init__(self, prefix):
        self.L = []
        self.prefix = prefix

    def e(self, t):
        self.L.append("  " + t)

    def all(self, ts):
        for t in ts:
            self.e(t)

    def ref(self, n):
        return ".L%s_%s_%%=" % (self.prefix, n)

    def lab(self, n):
        self.L.append(self.ref(n) + ":")


# ---- building blocks: lists of instructions

def frag_addrs(c, op):
    """LDS address register of every (operand, k-sub-step): sub-step 0 is the wrapper's operand, sub-step ks is that
    ^ (ks * 128 / NSUB) (the XOR swizzle only touches address bits 4..6: + ks 16-byte chunk groups = ^ under the swizzle),
    derived once into the registers behind the fragment sets.  Returns the map and the instructions that fill it."""
    vx = c.V0 + c.VN
    fa, xors = {("A", 0): op["faA0"], ("W", 0): op["faW0"]}, []
    for ks in range(1, c.NSUB):
        for x, r in (("A", vx + ks - 1), ("W", vx + c.NSUB - 1 + ks - 1)):
            fa[(x, ks)] = vr(r)
            xors.append("v_xor_b32_e32 %s, %d, %s" % (vr(r), ks * 128 // c.NSUB, fa[(x, 0)]))
    return fa, xors


def reads(c, fa, stage, ks, fset, word=0):
    """fragment reads of k-sub-step ks of `stage` into fragment set fset (from register `word` of every fragment on)"""
    out = []
    for x, n, first, size in (("A", c.NFA, 0, c.A_STAGE), ("W", c.NFW, c.NFA, c.W_STAGE)):
        for i in range(n):
            out.append("ds_read_b128 %s, %s offset:%d" % (vr(c.frag(fset, first + i) + word, 4), fa[(x, ks)], stage * size + i * c.FSTRIDE))
    return out


def mfmas(c, fset):
    """swapped operands: first = weight fragment (D rows = output channels), second = activation fragment (D columns = output
    rows).  16x16x32: a lane owns output row l % 16 and channels 4 (l / 16) .. + 3 of every 16 x 16 tile"""
    out = []
    for j in range(c.NFW):
        for i in range(c.NFA):
            acc = ar((j * c.NFA + i) * c.ACCW, c.ACCW)
            out.append("%s %s, %s, %s, %s" % (c.MFMA, acc, vr(c.frag(fset, c.NFA + j), c.FW), vr(c.frag(fset, i), c.FW), acc))
    return out


def offset_regs(c, op, sfx=""):
    return [op["aoff%s%d" % (sfx, i)] for i in range(c.NA)], [op["woff%s%d" % (sfx, i)] for i in range(c.NW)]


def dma(c, stage, aregs, wregs):
    """(M0 write, LDS-DMA load) pieces of this wave for one stage, from the per-lane source offsets aregs / wregs"""
    out = []
    for regs, dst, size, base in ((aregs, S_ADST, c.A_STAGE, S_AB), (wregs, S_WDST, c.W_STAGE, S_WB)):
        for i, r in enumerate(regs):
            out.append(("s_add_u32 m0, s%d, %d" % (dst, stage * size + i * c.DMA_STRIDE),
                        "global_load_lds_dwordx4 %s, s[%d:%d]" % (r, base, base + 1)))
    return out


def step_pointers():
    return ["s_add_u32 s%d, s%d, s%d" % (S_AB, S_AB, S_STEP),
            "s_addc_u32 s%d, s%d, 0" % (S_AB + 1, S_AB + 1),
            "s_add_u32 s%d, s%d, s%d" % (S_WB, S_WB, S_STEP),
            "s_addc_u32 s%d, s%d, 0" % (S_WB + 1, S_WB + 1)]


def next_step():
    """count the K step the loaders point at: S_STEP = its 128 bytes along K, 0 past the last one (they stay: harmless re-fetch);
    leaves scc = advancing"""
    return ["s_add_u32 s%d, s%d, 1" % (S_TMP, S_KL),
            "s_cmp_lt_u32 s%d, s%d" % (S_TMP, S_NK),
            "s_cselect_b32 s%d, 128, 0" % S_STEP,
            "s_cselect_b32 s%d, s%d, s%d" % (S_KL, S_TMP, S_KL)]


def advance():
    """point both loaders at the next K step"""
    return next_step() + step_pointers()


def conv_advance():
    """point the loaders at the next K step (tap-major): inside a tap the A base moves one channel block, at a
    tap boundary it returns to x and the table row changes; W is contiguous along K.  Past the last step: stay."""
    return next_step() + [
            "s_cselect_b32 s%d, 1, 0" % S_TMP,                           # 1 while advancing
            "s_add_u32 s%d, s%d, s%d" % (S_WB, S_WB, S_STEP),
            "s_addc_u32 s%d, s%d, 0" % (S_WB + 1, S_WB + 1),
            "s_add_u32 s%d, s%d, s%d" % (S_SIT, S_SIT, S_TMP),           # step inside the tap
            "s_cmp_ge_u32 s%d, s%d" % (S_SIT, S_NKT),                     # tap boundary?
            "s_cselect_b32 s%d, 0, s%d" % (S_SIT, S_SIT),
            "s_cselect_b32 s%d, 1024, 0" % S_STEP,
            "s_add_u32 s%d, s%d, s%d" % (S_TAPOFF, S_TAPOFF, S_STEP),
            "s_lshl_b32 s%d, s%d, 7" % (S_STEP, S_SIT),
            "s_add_u32 s%d, s%d, s%d" % (S_AB, S_XB2, S_STEP),
            "s_addc_u32 s%d, s%d, 0" % (S_AB + 1, S_XB2 + 1)]


def setup(op, pairs, words, zeros):
    """the asm-owned scalars: 64-bit and 32-bit copies of the wrapper's operands, counters"""
    return ["s_mov_b64 s[%d:%d], %s" % (s, s + 1, op[n]) for s, n in pairs] + \
           ["s_mov_b32 s%d, %s" % (s, op[n]) for s, n in words] + ["s_mov_b32 s%d, 0" % s for s in zeros]


def zero_acc(c):
    return ["v_accvgpr_write_b32 %s, 0" % ar(r) for r in range(c.NACC)]


def spread_slots(c, pieces, spread, block_reads, rd_per):
    """What rides in the shadow of every MFMA of a K step of len(block_reads) blocks of NFA x NFW MFMAs: LDS-DMA piece j behind
    MFMA j * spread with the NEXT piece's M0 write behind it (a piece's own M0 write sits one piece earlier: no s_nop in front of
    the load); the fragment reads of block b rd_per per shadow in the first shadows of block b that carry no piece (a
    ds_read_b128 costs ~9 cycles of a 16-cycle shadow).  Returns the slots and the index of the last piece's."""
    nm = c.NFA * c.NFW
    slots = [[] for _ in range(len(block_reads) * nm)]
    dma_slots = [spread * j for j in range(len(pieces))]
    for j, (m0w, d) in enumerate(pieces):
        slots[dma_slots[j]].append(d)
        if j + 1 < len(pieces):
            slots[dma_slots[j]].append(pieces[j + 1][0])
    for blk, rd in enumerate(block_reads):
        free = [i for i in range(blk * nm, (blk + 1) * nm) if i not in dma_slots]
        for i in range((len(rd) + rd_per - 1) // rd_per):
            slots[free[i]] += rd[rd_per * i: rd_per * i + rd_per]
    return slots, dma_slots[-1]


# ---- building blocks that emit

def plain(E, pieces):
    """LDS-DMA pieces outside MFMA shadows: the M0 write needs one wait state before the load reads it"""
    for m0w, d in pieces:
        E.e(m0w); E.e("s_nop 0"); E.e(d)


def shadowed(E, mf, pieces, spread=1):
    """one block of MFMAs with LDS-DMA piece j behind MFMA j * spread: M0 write before that MFMA (= behind the previous piece),
    load after it; pieces that find no shadow follow plainly"""
    E.e(pieces[0][0])
    for i, m in enumerate(mf):
        E.e(m)
        if i % spread == 0 and i // spread < len(pieces):
            j = i // spread
            E.e(pieces[j][1])
            if j + 1 < len(pieces):
                E.e(pieces[j + 1][0])
    plain(E, pieces[(len(mf) + spread - 1) // spread:])


def evenly(E, mf, items):
    """one block of MFMAs with the filler instructions spread evenly over their shadows"""
    per = [[] for _ in mf]
    for i, it in enumerate(items):
        per[i * len(mf) // len(items)].append(it)
    for m, f in zip(mf, per):
        E.e(m)
        E.all(f)


def trailing_step(E, c, cur, rd, pieces):
    """8-wave K step up to its entry point: fragment reads of sub-step 0, then the trailing sub-step of the previous K step
    (fragment set 1) with the LDS-DMA of the other stage in its shadows, then the loaders advance"""
    E.all(rd)
    shadowed(E, mfmas(c, 1), pieces)
    E.all(advance())
    E.lab("entry%d" % cur)


def two_block_step(E, c, cur, first_m0, slots, last, adv):
    """4-wave K step: the trailing block (k 32..63 of the previous K step, fragment set 1), then block 0 (set 0) behind the entry
    point, every MFMA followed by its slot (spread_slots); the loaders advance behind the last LDS-DMA piece"""
    nm = c.NFA * c.NFW
    E.e(first_m0)
    for blk in range(2):
        if blk == 1:
            E.lab("entry%d" % cur)
            E.e("s_waitcnt lgkmcnt(0)")
        for i, m in enumerate(mfmas(c, 1 if blk == 0 else 0)):
            E.e(m)
            E.all(slots[blk * nm + i])
            if blk * nm + i == last:
                E.all(adv)


def loop_tail(E, k, before_barrier=()):
    """end of K step k of the two-step loop body: everything landed, publish, count, leave or go round"""
    E.e("s_waitcnt vmcnt(0) lgkmcnt(0)")
    E.all(before_barrier)
    E.e("s_barrier")
    E.e("s_add_u32 s%d, s%d, 1" % (S_T, S_T))
    E.e("s_cmp_lt_u32 s%d, s%d" % (S_T, S_NK))
    E.e("s_cbranch_scc0 %s" % E.ref("exit"))
    if k == 1:
        E.e("s_branch %s" % E.ref("step0"))


def drain_exit(E, c):
    E.lab("exit")
    E.all(mfmas(c, 1))
    E.all(["s_nop 15", "s_nop 15"])


def pers_prologue(E, c, op, fa, xors, regs):
    """Entry of a persistent workgroup's tile (the asm statement is executed once per output tile of the workgroup's list):
      * flags bit 0 = stages 0 / 1 are already in flight (issued by the previous tile's exit): no load prologue;
      * the accumulators start from the bias (flags bit 2; ACCW f32 per MFMA-tile column and lane, loaded once per tile
        into the idle fragment registers, consumed before the first fragment read) instead of zero, so the epilogue of an
        un-gated Linear issues no load at all."""
    E.all(setup(op, [(S_AB, "abase"), (S_WB, "wbase"), (S_PBIAS, "bias")],
                [(S_NK, "nk"), (S_ADST, "adst"), (S_WDST, "wdst"), (S_PFLAGS, "flags")], [S_T, S_KL]))
    E.all(xors)

    def fetch_unless_in_flight(stage, label):
        E.e("s_bitcmp1_b32 s%d, %d" % (S_PFLAGS, PF_PREFETCHED))
        E.e("s_cbranch_scc1 %s" % E.ref(label))
        plain(E, dma(c, stage, *regs))
        E.lab(label)
        E.all(advance())

    fetch_unless_in_flight(0, "have0")
    E.e("s_bitcmp1_b32 s%d, %d" % (S_PFLAGS, PF_BIAS))
    E.e("s_cbranch_scc0 %s" % E.ref("nobias"))
    nq = c.ACCW // 4                           # bias quads per tile column block: channels 8 qd .. + 3 of a 32-wide tile, 0 .. 3 of a 16-wide
    for j in range(c.NFW):
        for qd in range(nq):
            E.e("global_load_dwordx4 %s, %s, s[%d:%d] offset:%d" % (vr(c.V0 + (j * nq + qd) * 4, 4), op["boff"], S_PBIAS, S_PBIAS + 1,
                                                                   (j * c.TILE + qd * 8) * 4))
    E.lab("nobias")
    E.e("s_waitcnt vmcnt(0)")
    E.e("s_barrier")
    fetch_unless_in_flight(1, "have1")
    E.e("s_bitcmp1_b32 s%d, %d" % (S_PFLAGS, PF_BIAS))
    E.e("s_cbranch_scc0 %s" % E.ref("zero"))
    for j in range(c.NFW):
        for i in range(c.NFA):
            for r in range(c.ACCW):
                E.e("v_accvgpr_write_b32 %s, %s" % (ar((j * c.NFA + i) * c.ACCW + r), vr(c.V0 + j * c.ACCW + r)))
    E.e("s_branch %s" % E.ref("inited"))
    E.lab("zero")
    E.all(zero_acc(c))
    E.lab("inited")
    E.e("s_nop 1")
    E.all(reads(c, fa, 0, 0, 0))
    E.e("s_branch %s" % E.ref("entry0"))


def pers_exit(E, c, op, next_regs, spread):
    """Exit of a persistent workgroup's tile: after the last barrier both LDS stages are free (every fragment of the last K step
    is in registers) -> the LDS-DMA of the NEXT tile's K steps 0 and 1 (flags bit 1 = there is one; per-lane offsets next_regs
    from the next tile's OWN 64-bit origins abasen / wbasen: every tile is addressed relative to its origin, so only a tile's
    256-row window has to fit the 32-bit lane offsets) is issued in the shadows of the trailing k-sub-step, so it lands
    while the wrapper runs this tile's epilogue."""
    E.lab("exit")
    E.e("s_bitcmp1_b32 s%d, %d" % (S_PFLAGS, PF_HAS_NEXT))
    E.e("s_cbranch_scc0 %s" % E.ref("last"))
    E.e("s_mov_b64 s[%d:%d], %s" % (S_AB, S_AB + 1, op["abasen"]))
    E.e("s_mov_b64 s[%d:%d], %s" % (S_WB, S_WB + 1, op["wbasen"]))
    shadowed(E, mfmas(c, 1), dma(c, 0, *next_regs), spread)
    E.e("s_cmp_gt_u32 s%d, 1" % S_NK)                      # K step 1 exists?  (else stage 1 re-fetches step 0: harmless)
    E.e("s_cselect_b32 s%d, 128, 0" % S_STEP)
    E.all(step_pointers())
    plain(E, dma(c, 1, *next_regs))
    E.e("s_branch %s" % E.ref("end"))
    E.lab("last")
    E.all(mfmas(c, 1))
    E.lab("end")
    E.all(["s_nop 15", "s_nop 15"])


# ---- the four shipped K loops

def gen_pers(c):
    """8-wave bf16 K loop for a PERSISTENT workgroup (csrc/gemm256p.hip; pers_prologue, pers_exit: the fixed costs of a tile move
    off the matrix pipe's critical path).  The next tile is fetched through its own offset operands aoffn / woffn.  One K step:
    reads of k-sub-step 0 | trailing k-sub-step 3 with one LDS-DMA piece per shadow | k-sub-steps 0..2, each with the reads of
    the next in its shadows."""
    assert not c.FP8 and c.BN == 128, "the shipped form: 4 MFMAs and 4 fragment reads per k-sub-step"
    E = Emit("p" + c.tag)
    fa, xors = frag_addrs(c, POP)
    regs = offset_regs(c, POP)
    pers_prologue(E, c, POP, fa, xors, regs)
    for k in range(2):
        E.lab("step%d" % k)
        trailing_step(E, c, k, reads(c, fa, k, 0, 0), dma(c, k ^ 1, *regs))
        for ks in range(3):
            fset = ks % 2
            E.e("s_waitcnt lgkmcnt(0)")
            evenly(E, mfmas(c, fset), reads(c, fa, k, ks + 1, fset ^ 1))
        loop_tail(E, k)
    pers_exit(E, c, POP, offset_regs(c, POP, "n"), 1)
    return E.L


def gen_x4(c, spread=4, rd_per=1):
    """4-wave persistent-workgroup K loop of Cfg4x (csrc/gemm256x.hip; pers_prologue, pers_exit).  Per K step and wave: 128 MFMAs
    of 16 cycles in two blocks of 64 -- the trailing sub-step (k 32..63 of the previous K step, fragment set 1) and sub-step 0
    (set 0) --, the 16 fragment reads of a block rd_per per shadow at its head, the 16 LDS-DMA pieces one per `spread` shadows
    of the trailing block (an LDS-DMA instruction holds the issue port for several MFMA shadows).  The per-lane source
    offsets are relative to the tile's own 64-bit origin (abase / wbase), and between two interior tiles they are equal -- so
    the exit fetches the next tile with THIS tile's offset registers from the next tile's origins (the wrapper clears flags
    bit 1 where either tile is not interior); the step between two origins does not have to fit 32 bits."""
    assert spread * (c.NA + c.NW - 1) < c.NFA * c.NFW, "all pieces are issued in the trailing block: entry0 re-issues none"
    E = Emit(c.tag)
    fa, xors = frag_addrs(c, WOP)
    regs = offset_regs(c, WOP)
    pers_prologue(E, c, WOP, fa, xors, regs)
    for k in range(2):
        E.lab("step%d" % k)
        pieces = dma(c, k ^ 1, *regs)
        slots, last = spread_slots(c, pieces, spread, [reads(c, fa, k, 0, 0), reads(c, fa, k, 1, 1)], rd_per)
        two_block_step(E, c, k, pieces[0][0], slots, last, advance())
        loop_tail(E, k)
    pers_exit(E, c, WOP, regs, spread)
    return E.L


def gen_fp8(c):
    """K loop of the fp8 (OCP e4m3) GEMM (csrc/gemm256.hip), one tile per workgroup: the 8-wave tile, LDS image (128-byte rows =
    128 K elements now) and LDS-DMA loaders; one v_mfma_f32_32x32x64_f8f6f4 (64 cycles, 2x the bf16 MAC rate) consumes what
    two consecutive bf16 k-sub-steps read: a 32-byte fragment = the 16-byte chunks (2 ks | hi) of k-sub-steps
    ks = 2 kp and 2 kp + 1.  (Which K element lands in which byte of the MFMA operand does not matter: activation
    and weight fragments are assembled identically, and a contraction is invariant under a common K permutation.)
    One K step of a wave = 2 k-sub-steps: reads of sub-step 0 | the trailing sub-step 1 of the previous K step with
    the LDS-DMA of the other stage in its shadows | sub-step 0 with the reads of sub-step 1 in its shadows |
    vmcnt(0) lgkmcnt(0), barrier."""
    assert c.FP8
    E = Emit(c.tag)
    fa = {(x, ks): OP["fa%s%d" % (x, ks)] for x in "AW" for ks in range(4)}
    regs = offset_regs(c, OP)

    def paired_reads(stage, kp, fset):
        return reads(c, fa, stage, 2 * kp, fset) + reads(c, fa, stage, 2 * kp + 1, fset, 4)

    E.all(setup(OP, [(S_AB, "abase"), (S_WB, "wbase")], [(S_NK, "nk"), (S_ADST, "adst"), (S_WDST, "wdst")], [S_T, S_KL]))
    E.all(zero_acc(c))
    # prologue: stage 0, then what step 0 does before its entry point (DMA of stage 1, reads of sub-step 0)
    plain(E, dma(c, 0, *regs))
    E.all(advance())
    E.e("s_waitcnt vmcnt(0)")
    E.e("s_barrier")
    plain(E, dma(c, 1, *regs))
    E.all(advance())
    E.all(paired_reads(0, 0, 0))
    E.e("s_branch %s" % E.ref("entry0"))
    for k in range(2):
        E.lab("step%d" % k)
        trailing_step(E, c, k, paired_reads(k, 0, 0), dma(c, k ^ 1, *regs))
        E.e("s_waitcnt lgkmcnt(0)")
        evenly(E, mfmas(c, 0), paired_reads(k, 1, 1))
        loop_tail(E, k)
    drain_exit(E, c)
    return E.L


def gen_conv_x4(c, spread=4):
    """The whole K axis (all filter taps) of the implicit-GEMM convolution (csrc/conv3d_256.hip) in ONE call, on gen_x4's
    compute side with gathered A rows.  K = taps x (Cin / 64) steps; inside a tap a step only advances the channel block
    (scalar base + 128 B), at a tap boundary every row slot takes a new voxel offset.  Those offsets sit in an LDS table
    [tap][256 rows] (4 B each, built by the wrapper before the call).  A wave's 8 activation pieces cover tile rows
    8 (wave + 4 i) + lane / 8: their voxel offsets sit 128 bytes apart in the table row of the tap (one address register +
    immediate offsets), and the swizzled channel-chunk offset is the same for all 8 (the row's swizzle key (r >> 1) & 7 does
    not depend on i).  Per K step: the 8 activation + NBJ weight LDS-DMA pieces one per `spread` shadows of the trailing
    block, then the loaders advance; the other block re-reads the offset table behind its fragment reads for the step they now
    point at, and the chunk offset is added behind the end-of-step wait (this step's pieces have long read their address
    registers)."""
    E = Emit("c" + c.tag)
    fa, xors = frag_addrs(c, CWOP)
    VA = c.V0 + c.VN + len(xors)   # table address of the tap being fetched
    VR = VA + 1                    # 8 raw table entries
    VO = VR + c.NA                 # 8 offsets of the step being fetched
    nm = c.NFA * c.NFW
    regs = [vr(VO + i) for i in range(c.NA)], [CWOP["woff%d" % i] for i in range(c.NW)]
    table_reads = ["v_add_u32_e32 %s, s%d, %s" % (vr(VA), S_TAPOFF, CWOP["arow0"])] + \
                  ["ds_read_b32 %s, %s offset:%d" % (vr(VR + i), vr(VA), i * 128) for i in range(c.NA)]
    table_adds = ["v_add_u32_e32 %s, %s, %s" % (vr(VO + i), vr(VR + i), CWOP["chk"]) for i in range(c.NA)]

    E.all(setup(CWOP, [(S_XB2, "xbase"), (S_AB, "xbase"), (S_WB, "wbase")],
                [(S_NK, "nk"), (S_NKT, "nkt"), (S_ADST, "adst"), (S_WDST, "wdst")], [S_T, S_KL, S_SIT, S_TAPOFF]))
    E.all(xors)
    E.all(zero_acc(c))
    # prologue: offsets of step 0, stage 0; then what step 0 does before its entry point
    E.all(table_reads)
    E.e("s_waitcnt lgkmcnt(0)")
    E.all(table_adds)
    E.e("s_nop 1")
    plain(E, dma(c, 0, *regs))
    E.all(conv_advance())
    E.all(table_reads)
    E.e("s_waitcnt vmcnt(0) lgkmcnt(0)")     # stage 0 landed AND its DMA has consumed the offset registers
    E.all(table_adds)
    E.e("s_barrier")
    E.e("s_nop 1")
    plain(E, dma(c, 1, *regs))
    first_entry_piece = (nm + spread - 1) // spread
    if first_entry_piece >= c.NA + c.NW:       # every piece is issued in the trailing block: entry0 re-issues none
        E.all(conv_advance())
    else:                                      # entry0 re-issues the pieces whose shadows lie behind it (same step, same offsets,
        E.e(dma(c, 1, *regs)[first_entry_piece][0])   # same data: the activation offsets are still this step's), then advances
    E.all(reads(c, fa, 0, 0, 0))
    E.e("s_branch %s" % E.ref("entry0"))
    for k in range(2):
        E.lab("step%d" % k)
        pieces = dma(c, k ^ 1, *regs)
        slots, last = spread_slots(c, pieces, spread, [reads(c, fa, k, 0, 0), reads(c, fa, k, 1, 1)], 1)
        # the table reads: block 1, behind its fragment reads and the loaders' advance
        base = max(max(i for i in range(nm, 2 * nm) if slots[i]), last) + 1
        assert base + 4 < 2 * nm
        slots[base] += table_reads[:3]
        for i in range(3, len(table_reads), 2):
            slots[base + 1 + (i - 3) // 2] += table_reads[i: i + 2]
        two_block_step(E, c, k, pieces[0][0], slots, last, conv_advance())
        loop_tail(E, k, table_adds)    # offsets of the step the loaders point at: this step's pieces were issued a block ago
    drain_exit(E, c)
    return E.L


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "open_sora_amd", "csrc"))
    args = ap.parse_args()

    def body(name, note, lines):
        write_body(os.path.join(args.out, name), SCRIPT, note, lines)

    def regs(name, text):
        with open(os.path.join(args.out, name), "w") as f:
            f.write(header(SCRIPT) + text)

    for bn in (256, 128):
        c = Cfg(bn)
        P = "OSKG%d_" % bn
        # accumulator tile t = AGPRs 16 t .. 16 t + 15 = quads 4 t .. 4 t + 3 (the wrappers bind them as asm outputs: acc_quads.h)
        regs("gemm256_regs_n%d.inc" % bn,
             "#define %sSMEM %d\n#define %sW_BASE %d\n#define %sTM %d\n#define %sTN %d\n" % (P, c.SMEM, P, c.W_BASE, P, c.TM, P, c.TN) +
             "#define %sCLOBBERS %s\n" % (P, clobbers(c.V0, c.VN, c.NACC, S_FIRST, S_LAST)) +
             "#define %sACC_QUADS %d\n" % (P, c.NACC // 4))
        q = Cfg(bn, fp8=True)
        body("gemm256_fp8_body_n%d.inc" % bn, "fp8 (e4m3) 256 x %d x 128 tile K loop." % bn, gen_fp8(q))
        regs("gemm256_fp8_regs_n%d.inc" % bn, "#define OSKQ%d_CLOBBERS %s\n" % (bn, clobbers(q.V0, q.VN, q.NACC, S_FIRST, S_LAST)))
    c = Cfg(128)
    body("gemm256p_body_n128_s0.inc", "256 x 128 x 64 tile K loop, persistent workgroup, schedule 0.", gen_pers(c))
    regs("gemm256p_regs_n128.inc", "#define OSKP128_CLOBBERS %s\n" % clobbers(c.V0, c.VN + 6, c.NACC, S_FIRST, PERS_S_LAST))
    cx, cx128 = Cfg4x(), Cfg4x(4)
    body("gemm256x_body.inc", "256 x 256 x 64 tile, 4 waves x (128 x 128) on v_mfma_f32_16x16x32_bf16, persistent workgroup.", gen_x4(cx))
    body("conv256x_body.inc", "256 x 256 x 64 tile, 4 waves x (128 x 128) on v_mfma_f32_16x16x32_bf16, whole K axis (all filter taps).",
         gen_conv_x4(cx))
    body("conv256x_body_n128.inc", "256 x 128 x 64 tile, 4 waves x (128 x 64) on v_mfma_f32_16x16x32_bf16, whole K axis (all filter taps).",
         gen_conv_x4(cx128))
    conv_v = lambda k: k.VN + 2 + 1 + 2 * k.NA      # fragment sets, 2 fragment addresses, table address, raw and final offsets
    # accumulator tile T = J * NB + I = AGPR quad T (the wrappers bind the quads as asm outputs: acc_quads.h)
    regs("gemm256x_regs.inc",
         "#define OSKX128_SMEM %d\n#define OSKX128_CONV_CLOBBERS %s\n" % (cx128.SMEM, clobbers(cx128.V0, conv_v(cx128), cx128.NACC, S_FIRST, CONV_S_LAST)) +
         "#define OSKX_SMEM %d\n#define OSKX_W_BASE %d\n#define OSKX_NB %d\n" % (cx.SMEM, cx.W_BASE, cx.NB) +
         "#define OSKX_CLOBBERS %s\n" % clobbers(cx.V0, cx.VN + 2, cx.NACC, S_FIRST, W4_S_LAST) +
         "#define OSKX_CONV_CLOBBERS %s\n" % clobbers(cx.V0, conv_v(cx), cx.NACC, S_FIRST, CONV_S_LAST) +
         "#define OSKX_ACC_QUADS %d\n#define OSKX128_ACC_QUADS %d\n" % (cx.NACC // 4, cx128.NACC // 4))


if __name__ == "__main__":
    main()
