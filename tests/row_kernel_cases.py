"""TEST INFRASTRUCTURE ONLY -- the cases, seeded CPU inputs, f64 expectations and acceptance checks of the row-kernel tests.

tests/test_gpu_row_kernels.py runs the HIP kernels on these inputs and hands their outputs to the check_* functions below;
tests/test_row_kernel_refs.py hands the SAME functions what the project's f32 oracle computes from the SAME inputs -- so every
tolerance here is shown, on a machine without a GPU, to admit the oracle's own f32 arithmetic and nothing looser.
Everything lives on the CPU; inputs come from oracle.synth with fixed seeds.
"""
from __future__ import annotations

import functools

import numpy as np
import torch

from oracle import synth
from tests import cpu_ops_rows_f64 as R
from tests.test_gpu_kernels import bf16_ulp_close

BF = torch.bfloat16
F64 = torch.float64
_PERIOD = 65521   # (prime) large tensors repeat one synth stream with this period: no row, chunk or tile size divides it


def rnd(name: str, shape, std: float = 1.0, seed: int = 7, dtype=BF, mean: float = 0.0) -> torch.Tensor:
    n = int(np.prod(shape))
    base = synth.normal(name, seed, (min(n, _PERIOD),), std=std, mean=mean)
    flat = base if n <= _PERIOD else np.resize(base, n)
    return torch.from_numpy(flat.reshape(shape).copy()).to(dtype)


def excess(got: torch.Tensor, ref: torch.Tensor, rel: float) -> float:
    """the absolute term a (rel, abs) comparison of got against ref needs: max(|got - ref| - rel |ref|) -- printed beside every check"""
    return float(((got.double() - ref.double()).abs() - rel * ref.double().abs()).max())


# ============================================================================================= LayerNorm + modulate
# class edges of the host's MAXC pick (chunks of 8 per lane: nch = ceil(D / 512) -> MAXC 1, 2, 3, 4, 6, 8), the one-chunk row
# and the maximum
LN_D = [8, 128, 512, 520, 1024, 1032, 1536, 1544, 2048, 2056, 3072, 3080, 4096]
LN_MAXC = {8: 1, 128: 1, 512: 1, 520: 2, 1024: 2, 1032: 3, 1536: 3, 1544: 4, 2048: 4, 2056: 6, 3072: 6, 3080: 8, 4096: 8}
LN_REFUSED_D = [4104, 12, 516]   # past the maximum; not a multiple of 8 (inside MAXC 1 and at a class edge)
LN_B, LN_L = 2, 37               # M = 74 rows: not a multiple of the 4 rows of a block
LN_REL, LN_ABS = 2.0 ** -7, 1e-3


@functools.lru_cache(maxsize=None)
def ln_case(D: int):
    """x: a row / column view inside a wider buffer; shift, scale: f32 views of one [B, 2 D + 8] modulation tensor"""
    B, L = LN_B, LN_L
    xbuf = rnd(f"ln.x{D}", (B, L + 3, D + 16), std=2.0, seed=211)
    x = xbuf[:, 2: 2 + L, 8: 8 + D]
    mod = rnd(f"ln.mod{D}", (B, 2 * D + 8), std=0.5, seed=212, dtype=torch.float32)
    c = dict(D=D, B=B, L=L, xbuf=xbuf, x=x, mod=mod, shift=mod[:, :D], scale=mod[:, D + 8: 2 * D + 8])
    if D <= 4096 and D % 8 == 0:
        c["ref"] = R.bf16(R.ln_modulate_f64(x, c["shift"], c["scale"]))
        c["ref8"] = R.ln_modulate_fp8_f64(x, c["shift"], c["scale"])
    return c


def check_ln(got: torch.Tensor, c) -> None:
    print(f"ln_modulate D={c['D']}: abs term needed {excess(got, c['ref'], LN_REL):.3e} (allowed {LN_ABS:.0e})")
    bf16_ulp_close(got.double(), c["ref"], rel=LN_REL, abs_=LN_ABS)


FP8_TIE_CAP = 0.005


def check_ln_fp8(q: torch.Tensor, s: torch.Tensor, c) -> None:
    """q uint8 [M, D], s f32 [M] against the f64 reference: scales bit-equal on every row whose absmax is not a bf16 tie; bytes
    equal, +-1 e4m3 code only on tie elements (and on rows whose scale a tie moved); excused elements <= 0.5 % of the case"""
    qr, sr, tie, amax_tie = c["ref8"]
    M, D = qr.shape
    same_scale = s == sr
    assert bool(same_scale[~amax_tie].all()), f"row scales differ on rows {torch.nonzero(~same_scale & ~amax_tie).flatten().tolist()[:8]}"
    excused = tie | (amax_tie & ~same_scale)[:, None]
    share = float(excused.float().mean())
    d = (R.e4m3_ordinal(q) - R.e4m3_ordinal(qr)).abs()
    n_diff, n_bad = int((d > 0).sum()), int(((d > 0) & ~excused).sum())
    print(f"ln_modulate_fp8 D={D}: {int(excused.sum())} of {M * D} elements excused as ties ({100 * share:.3f} %), "
          f"{n_diff} bytes differ, {n_bad} of them outside the excuse, {int((~same_scale).sum())} scales differ")
    assert share <= FP8_TIE_CAP, f"{100 * share:.3f} % of the elements are bf16 ties: choose other seeds"
    assert n_bad == 0, f"{n_bad} e4m3 bytes differ where the bf16 intermediate is no rounding tie"
    assert int(d.max()) <= 1, "an excused byte is more than one e4m3 code away"


# ============================================================================================= QK-RMSNorm + RoPE
QK_AXES = {64: [16, 24, 24], 72: [8, 32, 32], 128: [16, 56, 56]}
QK_THETA = 10000
QK_B, QK_L, QK_LT = 2, 37, 9    # 74 tokens: the blocks of every head count straddle the batch boundary, most end in a partial block
QK_H = [3, 4, 5, 7, 16, 24, 64, 65, 100, 128, 129, 256, 257]
QK_REL, QK_ABS, QK_ABS_MULT = 2.0 ** -7, 2e-3, 1e-3

# one factor at a time around the base call (q and k, per-batch tables, l_split = Lt, q_mult = 1, 16-byte aligned tables)
QK_VARIANTS = {
    "base": {},
    "q_only": dict(which="q"),
    "k_only": dict(which="k"),
    "csb0": dict(csb0=True),
    "lsplit0": dict(l_split=0),
    "lsplitL": dict(l_split=QK_L),
    "qmult": dict(qmult=True),
    "unaligned": dict(unaligned=True),                       # tables one float off 16 bytes: the lane-group kernel, same inputs as "base"
    "unaligned_qmult": dict(unaligned=True, qmult=True),     # ... same inputs as "qmult"
    "csb_odd": dict(csb_pad=1),                              # aligned tables, batch stride % 4 != 0: the lane-group kernel as well
    "rows": dict(rows=True),                                 # all-zero rows and rows with one x300 outlier
    "seqpar_k": dict(which="k", csb0=True),                  # the sequence-parallel path: K first, then Q with the softmax scale
    "seqpar_q": dict(which="q", csb0=True, qmult=True),
    "few_tokens": dict(B=1, L=3, Lt=1),                      # B * L below one block's tokens (H <= 42)
}
QK_SUBSET_H = [4, 6, 24, 129]


def qk_case_ids():
    """(H, hd, mode, variant) of every QK-norm case"""
    out = []
    for H in QK_H:
        for hd in (64, 72):
            for mode in (0, 1):
                out.append((H, hd, mode, "base"))
    for H in (3, 24):
        for mode in (0, 1):
            out.append((H, 128, mode, "base"))
            out.append((H, 128, mode, "qmult"))
    for H in QK_SUBSET_H:
        for hd in (72, 64):
            for mode in (0, 1):
                for v in QK_VARIANTS:
                    if v != "base" or H == 6:
                        out.append((H, hd, mode, v))
    return out


def _qk_ids(B: int, L: int, Lt: int) -> torch.Tensor:
    """positions [B, L, 3]: text tokens at 0, image tokens on a (t, h, w) grid, another grid origin per batch"""
    n = L - Lt
    g = torch.stack(torch.meshgrid(torch.arange(2), torch.arange(2), torch.arange((n + 3) // 4), indexing="ij"), -1).reshape(-1, 3)[:n].float()
    ids = torch.zeros(B, L, 3)
    for b in range(B):
        ids[b, Lt:] = g + 3.0 * b
    return ids


@functools.lru_cache(maxsize=8)
def _qk_tensor(H: int, hd: int, B: int, L: int):
    """the fused [B, L, 3 D] projection output inside a [B, L + 2, 3 D + 16] buffer (one row and 8 columns of guard band all
    round), and the four scale vectors"""
    D = H * hd
    big = rnd(f"qk.y{H}x{hd}", (B, L + 2, 3 * D + 16), std=1.5, seed=221)
    scales = tuple(rnd(f"qk.s{i}.{hd}", (hd,), std=0.2, seed=222, mean=1.0) for i in range(4))
    return big, scales


@functools.lru_cache(maxsize=8)
def _qk_tables(hd: int, mode: int, B: int, L: int, Lt: int, csb0: bool):
    ids = _qk_ids(B, L, Lt)
    if csb0:
        ids = ids[:1]
    axes = QK_AXES[hd]
    if mode == 0:   # everything in f64, the table is the cast (math.py rope)
        ang = R.rope_angles_f64(ids.reshape(-1, 3), axes, QK_THETA).reshape(ids.shape[0], L, hd // 2)
    else:           # f32 omega and f32 angles (math.py liger_rope)
        ang = torch.cat([ids[..., a, None] * (1.0 / (QK_THETA ** (torch.arange(0, d, 2, dtype=torch.float32) / d)))
                         for a, d in enumerate(axes)], -1)
    return ang, torch.cos(ang).float().contiguous(), torch.sin(ang).float().contiguous()


def qk_case(H: int, hd: int, mode: int, variant: str):
    v = QK_VARIANTS[variant]
    B, L, Lt = v.get("B", QK_B), v.get("L", QK_L), v.get("Lt", QK_LT)
    D = H * hd
    big0, scales = _qk_tensor(H, hd, B, L)
    big = big0.clone()
    y = big[:, 1: L + 1, 8: 8 + 3 * D]
    outlier = torch.zeros(B, L, H, dtype=torch.bool)
    if v.get("rows"):
        for t in (0, 1):   # q and k
            cols = y[:, :, t * D: (t + 1) * D]
            cols[0, 3, hd: 2 * hd] = 0                                   # a text row
            cols[B - 1, L - 1, (H - 1) * hd:] = 0                        # the very last row (the one every clamped index repeats)
            cols[0, 10, 5] *= 300.0                                      # head 0
            cols[B - 1, 20, D - 1] *= 300.0                              # head H - 1, last element
        outlier[0, 10, 0] = outlier[B - 1, 20, H - 1] = True
    l_split = v.get("l_split", Lt)
    q_mult = hd ** -0.5 * 1.4426950408889634 if v.get("qmult") else 1.0
    q_mult = float(torch.tensor(q_mult, dtype=torch.float32))            # as the kernel receives it
    ang, cos, sin = _qk_tables(hd, mode, B, L, Lt, bool(v.get("csb0")))
    which = v.get("which", "qk")
    refs = {}
    for t, name in enumerate("qk"):
        if name in which:
            refs[name] = R.qknorm_rope_f64(y[:, :, t * D: (t + 1) * D], scales[t], scales[2 + t], l_split, cos, sin, H, hd, mode,
                                           mult=q_mult if name == "q" else 1.0, with_ties=True)
    return dict(H=H, hd=hd, mode=mode, variant=variant, B=B, L=L, Lt=Lt, D=D, big=big, scales=scales, l_split=l_split, q_mult=q_mult,
                ang=ang, cos=cos, sin=sin, csb0=bool(v.get("csb0")), which=which, unaligned=bool(v.get("unaligned")), csb_pad=v.get("csb_pad", 0),
                outlier=outlier, refs=refs)


# share of a case's elements that may sit on a first-rounding tie.  Expected: a normalised value lies within 2^-18 relative of a
# boundary (boundaries 2^-8 .. 2^-7 relative apart) with probability ~ 2 * 2^-18 / 2^-7.5 = 0.14 %, either element of a pair
# ties both of its outputs: 0.28 %.  Measured over all cases: 0 .. 0.69 % (the top of the range on the 768-element cases).
QK_TIE_CAP = 0.01


def check_qk(got: torch.Tensor, c, name: str) -> None:
    """got [B, L, D] (any float dtype) against the f64 expectation of tensor `name` ('q' | 'k').  rel 2^-7 (one bf16 step) and the
    project's absolute terms: 2e-3, 1e-3 when q_mult folds the softmax scale in (outputs ~ hd^-1/2 smaller).  On a row with an
    x300 outlier the absolute term is scaled by the row's max |ref| (the normalised outlier is ~ sqrt(hd), not ~ 1).
    An element whose rotation pair holds a tie of the first rounding (cpu_ops_rows_f64.qknorm_rope_f64) is allowed what the tie
    rounded the other way moves it by; such elements are counted and capped at 1 % of the case.  (Measured on the CPU, f32
    oracle against the f64 reference, without that allowance: 3.97e-3 on single elements -- one bf16 step of a normalised value
    in [0.5, 1) that f32 rounds the other way -- where every other element needs below 2e-3.  A flat term would have to cover a
    step of the largest normalised value, 2^-6 or more, on every element.)"""
    ref, tied, extra = c["refs"][name]
    B, L, H, hd = c["B"], c["L"], c["H"], c["hd"]
    abs_ = QK_ABS_MULT if (name == "q" and c["q_mult"] != 1.0) else QK_ABS
    rowmax = ref.reshape(B, L, H, hd).abs().amax(-1)
    abs_t = torch.where(c["outlier"], abs_ * rowmax.clamp_min(1.0), torch.full_like(rowmax, abs_))[..., None]
    abs_t = abs_t.expand(B, L, H, hd).reshape(B, L, H * hd)
    d = (got.double() - ref).abs() - QK_REL * ref.abs()
    share = float(tied.float().mean())
    untied = float(d[~tied].max())
    print(f"qknorm {name} H={H} hd={hd} mode={c['mode']} {c['variant']}: abs term needed {untied:.3e} off the ties "
          f"(allowed {abs_:.0e}), {float(d.max()):.3e} with them; {int(tied.sum())} tied elements ({100 * share:.3f} %), "
          f"{int((tied & (d > abs_t)).sum())} of them use their allowance")
    assert share <= QK_TIE_CAP, f"{100 * share:.3f} % of the elements sit on first-rounding ties"
    bf16_ulp_close(got.double(), ref, rel=QK_REL, abs_=abs_t + extra)


# ============================================================================================= V transpose
VT_L = [1, 63, 64, 65, 150]
VT_B, VT_H = 2, 3


@functools.lru_cache(maxsize=None)
def vt_case(hd: int, L: int):
    D = VT_H * hd
    y = rnd(f"vt.y{hd}", (VT_B, L, 3 * D), seed=231)
    v = y[:, :, 2 * D:]
    return dict(hd=hd, L=L, y=y, v=v, Lp=(L + 63) // 64 * 64, ref=R.v_transpose_ref(v, VT_H, hd))


# ============================================================================================= GEMV task list
# (Bv, K, act_in): every LDS-slice class of the host -- 8 rows (K <= 2048, Bv > 4), 4 rows (K <= 4096), 1 row (K <= 16384) --
# at its edges, with batches that end in a partial slice
GEMV_CASES = [(9, 2048, 1), (9, 2048, 0), (3, 2048, 1), (5, 2056, 1), (5, 4096, 0), (5, 4096, 1), (2, 4104, 1), (2, 4104, 0),
              (2, 16384, 0), (1, 16384, 1), (2, 8, 1), (9, 8, 0)]
GEMV_REFUSED_K = [16392, 12]
# rows per layer: 1, RU - 1, RU, RU + 1 for both row unrolls (RU = 4 with 8-row slices, 8 otherwise), a whole 64-row task, 64 + 1
# and 64 + 36; three columns of the output between two layers belong to no task
GEMV_ROWS = [1, 3, 4, 5, 7, 8, 9, 64, 65, 100]
GEMV_GAP = 3
GEMV_ABS = 1e-4   # per unit of accumulation (|out| ~ 1)


@functools.lru_cache(maxsize=4)
def gemv_case(Bv: int, K: int, act_in: int):
    xbuf = rnd(f"gv.x{K}", (Bv, K + 8), seed=241, dtype=torch.float32)
    x = xbuf[:, :K]                                  # batch stride wider than the row
    layers, cols, col = [], [], 0
    for i, n in enumerate(GEMV_ROWS):
        w = rnd(f"gv.w{i}.{K}", (n, K), std=K ** -0.5, seed=242)
        b = rnd(f"gv.b{i}", (n,), std=0.1, seed=243) if i % 3 != 1 else None
        layers.append((w, b))
        cols.append(col)
        col += n + GEMV_GAP
    ncol = col
    c = dict(Bv=Bv, K=K, act_in=act_in, xbuf=xbuf, x=x, layers=layers, cols=cols, ncol=ncol)
    if K % 8 == 0 and K <= 16384:
        ref = torch.zeros(Bv, ncol, dtype=F64)
        covered = torch.zeros(ncol, dtype=torch.bool)
        for (w, _), c0, r in zip(layers, cols, R.gemv_f64(x, layers, act_in)):
            ref[:, c0: c0 + w.shape[0]] = r
            covered[c0: c0 + w.shape[0]] = True
        c.update(ref=ref, covered=covered)
    return c


def check_gemv(got: torch.Tensor, c, units: int = 1) -> None:
    """got f32 [Bv, ncol] (the task columns) after `units` accumulations of the same product"""
    cov = c["covered"]
    err = float((got.double()[:, cov] - units * c["ref"][:, cov]).abs().max())
    print(f"gemv Bv={c['Bv']} K={c['K']} act_in={c['act_in']} x{units}: max err {err:.3e} (allowed {units * GEMV_ABS:.0e})")
    assert err <= units * GEMV_ABS


# ============================================================================================= timestep embedding, RoPE tables
# (B, dim, time_factor, max_period): the default, an odd dim, time_factor 1, B * dim / 2 > 256 (several blocks), all three at once
TE_CASES = [(3, 256, 1000.0, 10000.0), (2, 33, 1000.0, 10000.0), (3, 64, 1.0, 10000.0), (5, 256, 1000.0, 10000.0), (7, 251, 37.5, 1000.0)]
TE_ABS = 2e-4   # f32 trig of arguments up to 1e3


@functools.lru_cache(maxsize=None)
def te_case(B: int, dim: int, tf: float, mp: float):
    t = torch.from_numpy(synth.uniform01("te.t", 251, B)).float()
    t[0] = 0.69921875
    if B > 2:
        t[1], t[2] = 0.0, 1.0
    return dict(t=t, dim=dim, tf=tf, mp=mp, ref=R.timestep_embedding_f64(t, dim, mp, tf))


def check_te(got: torch.Tensor, c) -> None:
    err = float((got.double() - c["ref"]).abs().max())
    print(f"timestep_embedding dim={c['dim']} tf={c['tf']}: max err {err:.3e} (allowed {TE_ABS:.0e})")
    assert err <= TE_ABS


ROPE_AXES = [[64], [16, 48], [8, 32, 32], [8, 8, 24, 24]]
ROPE_REFUSED_AXES = [[7, 32], [16, 24, 25], [8, 8, 8, 8, 8]]
ROPE_ROWS = 70
ROPE_ABS = 2e-5
# f32-angle mode (liger_rope): the angle pos * theta^(-2j/d) is formed in f32.  Its relative error: the exponent 2j/d rounded
# (2^-24) and amplified by ln(theta) = 9.2 in the power, powf (<= 2 ulp), the reciprocal and the product (2^-24 each) -- below
# 8 * 2^-23 together; cos / sin move by at most the angle's absolute error.  So the absolute term grows with |angle| * f32 epsilon.
ROPE_F32_ANGLE_REL = 8 * 2.0 ** -23


@functools.lru_cache(maxsize=None)
def rope_case(n_axes: int):
    axes = next(a for a in ROPE_AXES if len(a) == n_axes)
    i = torch.arange(ROPE_ROWS, dtype=torch.float32)
    ids = torch.zeros(ROPE_ROWS, n_axes)
    for a in range(n_axes):
        small = (i * (a + 1)) % (17 + 5 * a)                        # grid-sized positions ...
        large = 1000.0 + (50.0 + 3.0 * a) * i + 7.0 * a               # ... and positions in the thousands (720p grids), up to ~ 5e3
        ids[:, a] = torch.where(i < 40, small, large)
    ang = R.rope_angles_f64(ids, axes, QK_THETA)
    return dict(axes=axes, ids=ids, half=sum(axes) // 2, ang=ang, cos=torch.cos(ang), sin=torch.sin(ang))


def check_rope(cos: torch.Tensor, sin: torch.Tensor, c, f32_angles: bool) -> None:
    tol = ROPE_ABS + (ROPE_F32_ANGLE_REL * c["ang"].abs() if f32_angles else 0.0)
    for name, got, ref in (("cos", cos, c["cos"]), ("sin", sin, c["sin"])):
        d = (got.double() - ref).abs()
        print(f"rope_table {c['axes']} f32_angles={int(f32_angles)} {name}: max err {float(d.max()):.3e}, "
              f"as a share of the allowance {float((d / tol).max()):.3f}")
        assert bool((d <= tol).all())


# ============================================================================================= CFG + Euler
CFG_GRID = 2048 * 256 * 8    # elements one pass of the full grid covers
# (n, per-element g_img, in place)
CFG_CASES = {"scalar": (8000, False, False), "one_chunk": (8, True, False), "vec": (8000, True, False), "in_place": (8000, False, True),
             "in_place_vec": (8008, True, True), "grid_stride": (CFG_GRID + 8 * 1001, True, False)}
CFG_G_TXT, CFG_G_IMG, CFG_DT = 7.5, 3.0, -0.0321
CFG_REL, CFG_ABS = 2.0 ** -7, 1e-3


@functools.lru_cache(maxsize=2)
def cfg_case(name: str):
    n, vec, in_place = CFG_CASES[name]
    pred = rnd("cfg.p", (3, n), seed=261)
    x = rnd("cfg.x", (n,), seed=262)
    g = rnd("cfg.g", (n,), std=1.0, mean=3.0, seed=263, dtype=torch.float32) if vec else None
    return dict(n=n, pred=pred, x=x, g=g, in_place=in_place, ref=R.cfg_euler_f64(pred, x, CFG_G_TXT, g if vec else CFG_G_IMG, CFG_DT))


def check_cfg(got: torch.Tensor, c) -> None:
    print(f"cfg_euler n={c['n']}: abs term needed {excess(got, c['ref'], CFG_REL):.3e} (allowed {CFG_ABS:.0e})")
    bf16_ulp_close(got.double(), c["ref"], rel=CFG_REL, abs_=CFG_ABS)


# ============================================================================================= row copy
COPY_GRID = 4096 * 256       # 8-byte units one pass of the full grid covers
