"""TEST INFRASTRUCTURE ONLY -- operands, guard bands and the case table of the attention audit
(tests/test_attention_refs.py on the CPU, tests/test_gpu_attention_audit.py on the device).

Operands (built on the CPU from a seed, so both files see the same values):
  K, V   random; K rows are brought to unit RMS per head, as the model's QK-norm leaves them (|k|^2 = hd up to bf16 rounding).
         With plain unit-variance rows |k|^2 spreads over 72 +- 36 and no alpha gives every selector row a lead of 16 under a
         Cauchy-Schwarz bound of 56; with unit-RMS rows alpha = SEL_SCORE / hd does, for every head_dim (checked on the CPU).
  Q      three kinds of rows in every call:
         diffuse   random, a single key carries about 1 / Lk of the weight;
         selector  the MFMA's q = alpha * k[sel]: the selected score alpha |k|^2 = SEL_SCORE (44; GENERAL_SCORE = 70 for the
                   (batch, head) pairs an auto-dispatched call must hand to the general twin) leads every other by >= 16 in log2
                   units, so out ~= v[sel] and a dropped, duplicated, swapped or foreign key is an O(1) error in that row.
                   sel walks, in this order: the last valid key of every segment, the keys either side of every tail-part
                   boundary, every key of every segment's last tile, every key of the first tile (Case.wanted; the list is cut
                   where the call has too few rows, Operands.covered says so);
         special   the first selector row takes the last valid key of the last segment; the last row is all zero.
Guard bands (device side, layout()): every operand is a view inside one larger allocation; nothing sits at the end of one.
  Q rows outside [0, Lq) and K rows outside a segment are bf16 NaN, as are the gap columns; V^T / vt8 / k8 / the scale arrays have
  NaN guards around what the library's own preparation calls wrote (zero padding included); out has a row stride larger than
  H * hd; out, lse and the workspace surplus are prefilled with sentinel bit patterns.
"""
from __future__ import annotations

import dataclasses
import functools

import torch

from tests import cpu_ops_attn_f64 as R

BF = torch.bfloat16
SEL_SCORE = 44.0        # alpha * hd of a selector row on a FAST (batch, head): bound = 44 * (1 + rounding) < 56
GENERAL_SCORE = 70.0    # ... on a (batch, head) that must exceed the FAST limit
G = 8                   # guard rows either side of Q / K / out
SENT16 = 0x7FA5         # bf16 NaN
SENT32 = 0x7FA5A5A5     # f32 NaN
SENT8 = 0xA5


@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    api: str            # "bounded" (osk_attention_fwd_bounded_bf16), "auto", "pv8", "qk8"
    hd: int
    B: int
    H: int
    Lq: int
    n_seg: int
    seg: int
    Bkv: int = 0        # 0: every query batch has its own keys
    prescaled: bool = True
    fast: bool = False  # pass the Cauchy-Schwarz bound of the operands (bounded) -- the FAST body where the layout allows it
    split: int = 1      # key parts of the tail units: the workspace is sized for exactly this many (1: no workspace)
    wide: bool = False  # 512-row work units (attention_asm72w.hip), forced through osk_attention_rows_override
    fused: bool = False  # q (k, v where the call is a self-attention) as strided views of a [B, L, 3 D] buffer
    vslot: bool = False  # out into the dead V slot of that buffer
    body: str = "general"   # what attention_body must report ("FAST" / "general"); auto: both run

    @property
    def nb(self): return self.Bkv or self.B
    @property
    def D(self): return self.H * self.hd
    @property
    def segp(self): return (self.seg + 63) // 64 * 64
    @property
    def kind(self): return {"bounded": "bf16", "auto": "bf16", "pv8": "pv8", "qk8": "qk8"}[self.api]
    @property
    def rows(self): return 512 if self.wide else 256
    @property
    def units(self): return (self.Lq + self.rows - 1) // self.rows * self.B * self.H
    @property
    def ws_need(self): return self.units * self.split * self.rows * (self.hd + 1) * 4 if self.split > 1 else 0
    @property
    def klass(self):
        k = {"bounded": "asm128" if self.hd == 128 else ("asm72w" if self.wide else "asm72"), "auto": "auto",
             "pv8": f"asm{128 if self.hd == 128 else 72}p8", "qk8": "asm128q8"}[self.api]
        return f"{k} {self.body if self.api in ('bounded',) else ''}".strip()

    def parts(self):
        return R.key_parts(self.n_seg, self.seg, self.split)

    def wanted(self):
        """global key indices (segment s holds s * seg ..) the selector rows walk, most important first"""
        seg, n = self.seg, self.n_seg
        last = [s * seg + seg - 1 for s in reversed(range(n))]
        bnd = [x for a, _ in self.parts()[1:] for x in (a - 1, a)]
        tails = [s * seg + j for s in range(n) for j in range((self.segp // 64 - 1) * 64, seg)]
        first = list(range(min(64, seg)))
        return list(dict.fromkeys(last + bnd + tails + first))


def _c(name, api, hd, B, H, Lq, n_seg, seg, **kw):
    return Case(name, api, hd, B, H, Lq, n_seg, seg, **kw)


CASES = [
    # ---- asm72, general body (head_dim 72 and 64)
    _c("g72_1tile_ragged", "bounded", 72, 2, 2, 33, 1, 37),
    _c("g72_2tiles_plain", "bounded", 72, 1, 3, 257, 1, 65, prescaled=False),
    _c("g72_short_segments_fallback_merge", "bounded", 72, 2, 2, 300, 3, 128, Bkv=1, fast=True, split=3),
    _c("g72_1tile_segments", "bounded", 72, 1, 2, 255, 2, 63),
    _c("g64_tile_runs_merge64", "bounded", 64, 1, 2, 31, 1, 192, split=3),
    _c("g72_6tiles_ragged_last_part", "bounded", 72, 1, 2, 256, 1, 321, split=2),
    # ---- asm72, FAST body
    _c("f72_one_key", "bounded", 72, 2, 2, 1, 1, 1, fast=True, body="FAST"),
    _c("f72_5tiles_fused_vslot", "bounded", 72, 1, 3, 300, 1, 300, fast=True, fused=True, vslot=True, body="FAST"),
    _c("f64_whole_tile_plain", "bounded", 64, 2, 2, 256, 1, 64, fast=True, prescaled=False, body="FAST"),
    _c("f72_ragged_segments_shared_merge", "bounded", 72, 2, 1, 257, 2, 129, Bkv=1, fast=True, split=2, body="FAST"),
    _c("f64_5_segments_merge", "bounded", 64, 1, 2, 33, 5, 129, fast=True, split=5, body="FAST"),
    _c("f72_one_tile_per_part", "bounded", 72, 1, 2, 255, 1, 128, fast=True, split=2, body="FAST"),
    _c("f72_6tiles", "bounded", 72, 1, 2, 31, 1, 321, fast=True, body="FAST"),
    # ---- asm72w (512-row units), FAST body
    _c("w72_2tiles", "bounded", 72, 1, 2, 1024, 1, 65, fast=True, wide=True, body="FAST"),
    _c("w64_3tiles_merge", "bounded", 64, 1, 2, 1025, 1, 192, fast=True, wide=True, split=3, body="FAST"),
    _c("w72_wave_past_lq_segments", "bounded", 72, 1, 1, 1100, 2, 300, fast=True, wide=True, split=2, body="FAST"),
    _c("w64_1tile_plain", "bounded", 64, 2, 1, 1024, 1, 37, fast=True, wide=True, prescaled=False, body="FAST"),
    # ---- asm128, general body
    _c("g128_1tile_ragged", "bounded", 128, 2, 2, 33, 1, 63),
    _c("g128_3tiles_plain_merge128", "bounded", 128, 1, 2, 257, 1, 129, prescaled=False, split=3),
    _c("g128_short_segments_fallback", "bounded", 128, 2, 1, 300, 2, 65, Bkv=1, fast=True, split=2),
    _c("g128_fused_vslot", "bounded", 128, 1, 3, 256, 1, 256, fused=True, vslot=True),
    # ---- asm128, FAST body
    _c("f128_whole_tile", "bounded", 128, 1, 2, 255, 1, 64, fast=True, body="FAST"),
    _c("f128_5tiles_plain", "bounded", 128, 2, 2, 31, 1, 300, fast=True, prescaled=False, body="FAST"),
    _c("f128_segments_merge", "bounded", 128, 1, 2, 300, 3, 192, fast=True, split=3, body="FAST"),
    _c("f128_6tiles_ragged_last_part", "bounded", 128, 1, 2, 256, 1, 321, fast=True, split=2, body="FAST"),
    _c("f128_one_row", "bounded", 128, 2, 1, 1, 1, 128, fast=True, body="FAST"),
    # ---- fp8 P.V
    _c("p72_1tile_ragged", "pv8", 72, 2, 2, 33, 1, 37, prescaled=False),
    _c("p72_shared_prescaled_fused", "pv8", 72, 2, 2, 300, 2, 150, Bkv=1, fused=True),
    _c("p72_merge", "pv8", 72, 1, 2, 257, 1, 300, prescaled=False, split=5),
    _c("p128_2tiles_plain", "pv8", 128, 1, 2, 255, 1, 65, prescaled=False),
    _c("p128_shared_prescaled_fused_merge", "pv8", 128, 2, 2, 256, 3, 129, Bkv=1, fused=True, split=3),
    _c("p128_6tiles", "pv8", 128, 1, 1, 31, 1, 321),
    # ---- fp8 QK^T + fp8 P.V
    _c("q128_1tile_ragged_plain", "qk8", 128, 1, 2, 33, 1, 63, prescaled=False),
    _c("q128_shared_segments_merge", "qk8", 128, 2, 2, 300, 2, 192, Bkv=1, split=2),
    _c("q128_tile_runs_merge", "qk8", 128, 1, 2, 257, 1, 300, prescaled=False, split=5),
    # ---- auto-dispatched pair: (batch, head) bounds on both sides of 56
    _c("a72_pair_merge", "auto", 72, 2, 2, 300, 1, 300, split=5, body="pair"),
    _c("a64_pair_segments", "auto", 64, 1, 2, 257, 3, 192, body="pair"),
    _c("a128_pair_shared_merge", "auto", 128, 2, 2, 255, 1, 129, Bkv=1, split=3, body="pair"),
    _c("aw72_pair_wide", "auto", 72, 1, 2, 1024, 1, 128, wide=True, body="pair"),
]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


@dataclasses.dataclass
class Operands:
    q: torch.Tensor          # bf16 [B, Lq, D] as stored
    k: torch.Tensor          # bf16 [n_seg, nb, seg, D]
    v: torch.Tensor
    sel: torch.Tensor        # long [B, H, Lq]: the selected global key of a selector row, -1 otherwise
    covered: bool
    bound: float             # Cauchy-Schwarz bound of the MFMA operands over the call (log2 units)
    k_scale: torch.Tensor | None
    v_scale: torch.Tensor | None
    qm: torch.Tensor         # MFMA operands (f32): [B, H, Lq, hd], [nb, H, Lk, hd] x 2
    km: torch.Tensor
    vm: torch.Tensor


def general_pair(case: Case, b: int, h: int) -> bool:
    """auto-dispatched calls: does (b, h) get operands whose bound exceeds the FAST limit?  Both kinds in every call."""
    return case.api == "auto" and (b + h) % 2 == 1


@functools.lru_cache(maxsize=None)
def operands(name: str) -> Operands:
    c = BY_NAME[name]
    g = torch.Generator().manual_seed(1000 + CASES.index(c))
    hd, H, D, nb = c.hd, c.H, c.D, c.nb
    scale = hd ** -0.5
    k = torch.randn(c.n_seg, nb, c.seg, H, hd, generator=g)
    k = (k * torch.rsqrt(k.pow(2).mean(-1, keepdim=True))).reshape(c.n_seg, nb, c.seg, D).to(BF)
    v = torch.randn(c.n_seg, nb, c.seg, D, generator=g).to(BF)
    k_scale = R.fp8_scales(k, H, hd) if c.kind == "qk8" else None
    v_scale = R.fp8_scales(v, H, hd) if c.kind != "bf16" else None
    sc = 1.0 if c.prescaled else float(R.kernel_sc(scale))
    # MFMA-unit target rows, then / sc for a plain call (whose fold multiplies by sc again)
    qt = torch.randn(c.B, H, c.Lq, hd, generator=g) * (scale * R.LOG2E)
    kall = k.float().permute(1, 0, 2, 3).reshape(nb, c.n_seg * c.seg, H, hd).permute(0, 2, 1, 3)    # [nb, H, Lk, hd]
    sel = torch.full((c.B, H, c.Lq), -1, dtype=torch.long)
    slots = [(b, h, r) for r in range(c.Lq) for b in range(c.B) for h in range(H) if r % 4 != 3]
    wanted = c.wanted()
    zero = slots.pop() if len(slots) >= 2 else None
    for i, (b, h, r) in enumerate(slots):
        key = wanted[i % len(wanted)]
        alpha = (GENERAL_SCORE if general_pair(c, b, h) else SEL_SCORE) / hd
        qt[b, h, r] = alpha * kall[b % nb, h, key]
        sel[b, h, r] = key
    if zero is not None:
        qt[zero] = 0.0
    q = (qt / sc).permute(0, 2, 1, 3).reshape(c.B, c.Lq, D).to(BF)
    qm = R.mfma_q(q, H, hd, scale, c.prescaled, c.kind)
    km = R.mfma_k(k, H, hd, c.kind, k_scale)
    vm = R.mfma_v(v, H, hd, c.kind, v_scale)
    bound = float(qm.norm(dim=-1).amax() * km.norm(dim=-1).amax()) * 1.001
    return Operands(q, k, v, sel, len(slots) >= len(wanted), bound, k_scale, v_scale, qm, km, vm)


@functools.lru_cache(maxsize=None)
def reference(name: str) -> dict:
    """the f64 result and tolerances of a case: computed once, shared by every test that needs it, never modified"""
    o = operands(name)
    return R.reference(o.qm, o.km, o.vm, "bf16" if BY_NAME[name].kind == "bf16" else "fp8")


def emulation_modes(case: Case, ops: Operands):
    """the reference points an emulation of this case's kernel class runs at"""
    if case.api == "auto":
        return ["max", "max-8", 56.0]
    return [ops.bound] if case.body == "FAST" else ["max", "max-8"]


# =============================================================================================== device side
def _nan16(*shape, device):
    return torch.full(shape, SENT16, dtype=torch.int16, device=device).view(BF)


def _flat_guarded(n_seg, per, gap, dtype, fill, device):
    """n_seg tensors of `per` elements, per + gap apart, inside one allocation with guards in front and behind"""
    stride = per + gap
    buf = torch.full((2 * gap + n_seg * stride,), fill, dtype=torch.int16 if dtype == BF else dtype, device=device)
    buf = buf.view(BF) if dtype == BF else buf
    return buf, [buf[gap + s * stride: gap + s * stride + per] for s in range(n_seg)], stride


def _guarded_f32(t, device):
    buf = torch.full((t.numel() + 32,), SENT32, dtype=torch.int32, device=device).view(torch.float32)
    view = buf[16:16 + t.numel()].view(t.shape)
    view.copy_(t)
    return buf, view


def layout(lib, case: Case, ops: Operands, device, packed: bool = False) -> dict:
    """the device operands of one call.  packed: tightly packed tensors of their own (the twin call the guarded one must equal bit
    for bit); otherwise every operand is a view with guard bands as the module docstring says.  Returns the call's tensors plus
    `frozen`: (buffer, written view or None) pairs whose bytes outside the view must not change during the attention call."""
    c, D, hd, H, nb = case, case.D, case.hd, case.H, case.nb
    g = 0 if packed else G
    fused = c.fused and not packed
    selfattn = fused and c.Lq == c.seg and c.n_seg == 1 and nb == c.B
    W = 3 * D if fused else (D if packed else D + 16)
    q0 = 0 if (fused or packed) else 8
    L = {}
    qbuf = _nan16(c.B, g + c.Lq + g, W, device=device)
    q = qbuf[:, g:g + c.Lq, q0:q0 + D]
    q.copy_(ops.q)
    if selfattn:
        kbuf = qbuf[None]
        kv = qbuf[None, :, g:g + c.seg, D:2 * D]
        vv = qbuf[None, :, g:g + c.seg, 2 * D:3 * D]
        kv.copy_(ops.k), vv.copy_(ops.v)
    else:
        kbuf = _nan16(c.n_seg, nb, g + c.seg + g, W, device=device)
        k0 = D if fused else q0
        kv = kbuf[:, :, g:g + c.seg, k0:k0 + D]
        kv.copy_(ops.k)
        vv = ops.v.to(device)
    frozen = [[qbuf, None]] + ([] if selfattn else [[kbuf, None]])
    # V^T (and K) in the kernels' own layouts, written by the library's preparation calls into guarded allocations
    gap = 0 if packed else 64
    if c.kind == "bf16":
        vbuf, vts, vstride = _flat_guarded(c.n_seg, nb * H * hd * c.segp, gap, BF, SENT16, device)
        for s_ in range(c.n_seg):
            lib.v_transpose(vv[s_], vts[s_].view(nb, H, hd, c.segp), H, hd)
        L.update(vt=vts[0].view(nb, H, hd, c.segp), vt_seg_stride=vstride)
    else:
        rp = lib.vt8_rows(hd)
        sbuf, v_scale = _guarded_f32(ops.v_scale, device)
        vbuf, vts, vstride = _flat_guarded(c.n_seg, nb * H * rp * c.segp, gap, torch.uint8, 0x7F, device)
        for s_ in range(c.n_seg):
            lib.v_transpose_fp8(vv[s_], v_scale, vts[s_].view(nb, H, rp, c.segp), H, hd)
        L.update(vt=vts[0].view(nb, H, rp, c.segp), vt_seg_stride=vstride, v_scale=v_scale)
        frozen.append([sbuf, None])
    frozen.append([vbuf, None])
    if c.kind == "qk8":
        ksbuf, k_scale = _guarded_f32(ops.k_scale, device)
        k8buf, k8s, k8stride = _flat_guarded(c.n_seg, nb * H * c.segp * 128, gap, torch.uint8, 0x7F, device)
        for s_ in range(c.n_seg):
            lib.k_pack_fp8(kv[s_], k_scale, k8s[s_].view(nb, H, c.segp, 128), H, hd)
        L.update(k8=k8s[0].view(nb, H, c.segp, 128), k8_seg_stride=k8stride, k_scale=k_scale)
        frozen += [[ksbuf, None], [k8buf, None]]
    if c.api == "auto":
        n2 = torch.full((2, max(c.B, nb) * H + 32), SENT32, dtype=torch.int32, device=device).view(torch.float32)
        qn2, kn2 = n2[0, 16:16 + c.B * H].view(c.B, H), n2[1, 16:16 + nb * H].view(nb, H)
        lib.rownorm2_max(q, qn2, H, hd)
        for s_ in range(c.n_seg):
            lib.rownorm2_max(kv[s_], kn2, H, hd, accumulate=s_ > 0)
        L.update(qn2=qn2, kn2=kn2)
        frozen.append([n2, None])
    # results
    if c.vslot and fused:
        out = qbuf[:, g:g + c.Lq, 2 * D:3 * D]
        frozen[0][1] = out
    else:
        Wo = D if packed else D + 8
        obuf = torch.full((c.B, g + c.Lq + g, Wo), SENT16, dtype=torch.int16, device=device).view(BF)
        out = obuf[:, g:g + c.Lq, (0 if packed else 4):(0 if packed else 4) + D]
        frozen.append([obuf, out])
    lbuf = torch.full((c.B * H * c.Lq + 32,), SENT32, dtype=torch.int32, device=device).view(torch.float32)
    lse = lbuf[16:16 + c.B * H * c.Lq].view(c.B, H, c.Lq)
    frozen.append([lbuf, lse])
    ws = None
    if c.split > 1:
        # sized for exactly `split` parts (+ 512 bytes, less than any further part needs); a further 4096 sentinel bytes lie behind
        # what the call is told about
        wbuf = torch.full((c.ws_need + 512 + 4096,), SENT8, dtype=torch.uint8, device=device)
        ws = wbuf[:c.ws_need + 512]
        frozen.append([wbuf, wbuf[:c.ws_need]])
    L.update(q=q, k=kv[0], k_seg_stride=kbuf.stride(0), out=out, lse=lse, ws=ws, frozen=frozen)
    return L


def dispatch(lib, case: Case, ops: Operands, ws_bytes: int):
    """(body name, key parts, rows per unit) the library reports for this call"""
    c = case
    bound = ops.bound if c.fast else (1.0 if c.api == "auto" else 0.0)
    if c.api in ("pv8", "qk8"):
        return "general", lib.lib.osk_attention_tail_split_factor(c.B, c.H, c.Lq, c.n_seg, c.seg, c.hd, ws_bytes), 256
    parts, rows = lib.attention_launch_shape(c.B, c.H, c.Lq, c.n_seg, c.seg, c.hd, bound, ws_bytes)
    body = lib.attention_body(c.hd, c.n_seg, c.seg, bound)
    return ("FAST" if "FAST" in body else "general"), parts, rows


def call(lib, case: Case, ops: Operands, L: dict):
    c = case
    kw = dict(lse=L["lse"], n_seg=c.n_seg, seg_len=c.seg, vt_seg_stride=L["vt_seg_stride"], q_prescaled=c.prescaled,
              kv_batches=c.Bkv, workspace=L["ws"])
    scale = c.hd ** -0.5
    if c.api == "bounded":
        lib.attention_fwd(L["q"], L["k"], L["vt"], L["out"], c.H, c.hd, scale, k_seg_stride=L["k_seg_stride"],
                          score_bound=ops.bound if c.fast else 0.0, **kw)
    elif c.api == "auto":
        lib.attention_fwd_auto(L["q"], L["k"], L["vt"], L["out"], c.H, c.hd, scale, L["qn2"], L["kn2"],
                               k_seg_stride=L["k_seg_stride"], **kw)
    elif c.api == "pv8":
        lib.attention_fwd_pv8(L["q"], L["k"], L["vt"], L["v_scale"], L["out"], c.H, c.hd, scale, k_seg_stride=L["k_seg_stride"], **kw)
    else:
        lib.attention_fwd_qk8(L["q"], L["k8"], L["k_scale"], L["vt"], L["v_scale"], L["out"], c.H, c.hd, scale,
                              k_seg_stride=L["k8_seg_stride"], **kw)


def _bits(t):
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


def snapshot(L: dict):
    return [buf.clone() for buf, _ in L["frozen"]]


def disturbed(L: dict, before) -> list:
    """indices of the guarded allocations with a changed byte outside the view the call may write"""
    bad = []
    for i, ((buf, view), old) in enumerate(zip(L["frozen"], before)):
        if view is not None:     # put the old bytes back under the written view of a COPY, then the whole allocation must be as before
            now = buf.clone()
            off = view.storage_offset() - buf.storage_offset()
            torch.as_strided(now, view.shape, view.stride(), off).copy_(torch.as_strided(old, view.shape, view.stride(), off))
        else:
            now = buf
        if not torch.equal(_bits(now), _bits(old)):
            bad.append(i)
    return bad
