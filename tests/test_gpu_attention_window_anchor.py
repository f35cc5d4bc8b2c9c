"""GPU: frame-window attention with anchor frames (osk_attention_fwd_window_anchor_bf16) and the three-part in-place merge
(osk_attention_merge_into2_bf16).  (1) The merge per element against f64 with the bound tests/test_gpu_attention_merge.py derives,
rows with one, two and all three parts at -inf in one tensor, `out` a strided view inside guard bands.  (2) The entry against the f64
reference over each block's stated key set (prefix, run, suffix; tests/cpu_ops_window_anchor.py, e4m3 operands in the fp8 modes) in
every mode, on a geometry whose frames are no multiple of the tile and on a tile-aligned one, Lq != Lk through a row slice that is no
multiple of 256 rows.  (3) The mask exactly: with V the indicator of a key's part an output dim IS the softmax mass on that part.
(4) n_suffix = 0 bit for bit the window entries.  (5) Refused arguments.  (6) Capture and replay.  (7) The model: anchors that
cover all but one frame agree with the window off, anchors move a W = 0 forward, and the sharded forward (ranks as threads, both
exchange modes, aligned and ragged) is the single-device anchored forward.  Each check prints its figures before it asserts."""
import functools

import pytest
import torch

from tests import cpu_ops_window_anchor as A
from tests.cpu_ops_sp_chunked import attention_merge_f64
from tests.test_attention_window_fp8_host import packed
from tests.test_gpu_seqpar_ragged import _Counting, _ranks_forward
from tests.test_gpu_seqpar_window import _gpu_model
from tests.util import rel_l2, torch_inputs

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF = torch.bfloat16
R = A.R
H_, B_ = 2, 2
NEG_INF = float("-inf")
# (L_txt, N, T): 64 + 6 x 96 = 640 keys -- anchors (1, 0): n_prefix 192 takes in 32 keys of frame 1; (0, 1): s0 = 512, n_suffix 128
# takes in 32 keys of frame 4 -- and the tile-aligned 128 + 5 x 128 = 768
GEOMS = {"g1": (64, 96, 6), "g2": (128, 128, 5)}
ROW0 = 100                                       # a query slice [100, L): 540 / 668 rows, blocks that start off the 256-row grid
# (mode, hd, FAST): every body the window runs in today
MODES = [("bf16", 64, False), ("bf16", 72, False), ("bf16", 128, False), ("bf16", 72, True), ("bf16", 128, True),
         ("pv8", 72, False), ("pv8", 128, False), ("qk8", 128, False)]
G1_CASES = [(a, w, sl) for a in ((1, 0), (0, 1), (1, 1)) for w, sl in ((0, False), (1, True))]


@functools.lru_cache(maxsize=None)
def _operands(hd: int, L: int):
    return A.operands(hd, H_, B_, B_, L)         # q (prescaled), k, v, a score bound that holds


@functools.lru_cache(maxsize=None)
def _case(kind: str, hd: int, geom: str, anchors, Wf: int, sliced: bool):
    """(q rows, k, v, bound, n_prefix, n_suffix, table, reference): computed once per process, shared, read-only"""
    from open_sora_amd.mmdit import attention_window_bounds, attention_window_table

    L_txt, N, T = GEOMS[geom]
    L = L_txt + N * T
    q, k, v, sb = _operands(hd, L)
    row0 = ROW0 if sliced else 0
    n_prefix, n_suffix = attention_window_bounds(L_txt, N * T, N, *anchors)
    t = attention_window_table(L_txt, N * T, N, Wf, row0=row0, n_rows=L - row0, anchor_head=anchors[0], anchor_tail=anchors[1])
    qs = q[:, row0:].contiguous()
    return qs, k, v, sb, n_prefix, n_suffix, t, A.reference3(qs, k, v, H_, hd, n_prefix, n_suffix, t, kind)


def _vt(hip_lib, v, hd):
    vt = torch.zeros(v.shape[0], H_, hd, (v.shape[1] + 63) // 64 * 64, dtype=BF, device=DEV)
    hip_lib.v_transpose(v, vt, H_, hd)
    return vt


def _prepare(hip_lib, k, v, hd, kind):
    """device operands of the mode as keyword-free (k, vt, extra keywords)"""
    if kind == "bf16":
        return k.to(DEV), _vt(hip_lib, v.to(DEV), hd), {}
    kk, sk, vt8, sv = packed(hip_lib, k, v, hd, kind, DEV)
    return kk, vt8, dict(k_scale=sk, v_scale=sv, Lk=k.shape[1])


def _run(hip_lib, q, kd, vt, kw, hd, kind, table, n_prefix, n_suffix, bound=0.0, lse=True):
    out = torch.full_like(q, float("nan"))
    l = torch.full((q.shape[0], H_, q.shape[1]), float("nan"), device=DEV) if lse else None
    hip_lib.attention_fwd_window_anchor(q, kd, vt, out, H_, hd, hd ** -0.5, n_prefix=n_prefix, n_suffix=n_suffix, windows=table, mode=kind,
                                        lse=l, q_prescaled=True, score_bound=bound, **kw)
    torch.cuda.synchronize()
    return out.cpu(), None if l is None else l.cpu()


# ----------------------------------------------------------------------------- 1. the three-part merge
def _merge_case(hip_lib, hd, seed):
    B, H, Lq = 2, 2, 300
    D, Lqp = H * hd, 512
    g = torch.Generator().manual_seed(seed)
    parts = (torch.randn(3, B, Lq, D, generator=g) * 1.5)
    parts[0] = parts[0].to(BF).float()                                   # the finished rows are bf16, the partials f32
    lse = torch.randn(3, B, H, Lq, generator=g) * 2.0 + 5.0
    for s in range(3):                                                   # one part empty: rows 7 s + 1 mod 21
        lse[s, :, :, 7 * s + 1::21] = NEG_INF
    lse[0, :, :, 3::21], lse[1, :, :, 3::21] = NEG_INF, NEG_INF          # two parts empty, each pair
    lse[0, :, :, 4::21], lse[2, :, :, 4::21] = NEG_INF, NEG_INF
    lse[1, :, :, 5::21], lse[2, :, :, 5::21] = NEG_INF, NEG_INF
    lse[:, :, :, 6::21] = NEG_INF                                        # all three
    lse[1, 0, 0, 20] += 60.0                                             # one part far ahead: the others underflow
    exact, lse_exact, mag = attention_merge_f64(parts.double(), lse)
    # out: a strided view (rows wider than D) inside guard bands; the partials [B, H, Lqp, hd] with rows >= Lq poisoned
    obuf = torch.full((B + 2, Lq + 2, D + 64), -3.0, dtype=BF, device=DEV)
    out = obuf[1:B + 1, 1:Lq + 1, 32:32 + D]
    out.copy_(parts[0].to(DEV))
    lbuf = torch.full((B * H * Lq + 64,), 123.0, device=DEV)
    la = lbuf[32:32 + B * H * Lq].view(B, H, Lq)
    la.copy_(lse[0].to(DEV))
    ob, oc = (torch.full((B, H, Lqp, hd), float("nan"), device=DEV) for _ in range(2))
    lb, lc = (torch.full((B, H, Lqp), float("nan"), device=DEV) for _ in range(2))
    for o_, l_, s in ((ob, lb, 1), (oc, lc, 2)):
        o_[:, :, :Lq] = parts[s].reshape(B, Lq, H, hd).permute(0, 2, 1, 3).to(DEV)
        l_[:, :, :Lq] = lse[s].to(DEV)
        dead = torch.isinf(lse[s])[..., None].expand(B, H, Lq, hd)
        o_[:, :, :Lq][dead.to(DEV)] = float("nan")                      # a part without mass may hold anything
    assert out.stride(1) == D + 64 and out.data_ptr() % 16 == 0
    hip_lib.attention_merge_into2(out, la, ob, lb, oc, lc, H, hd)
    torch.cuda.synchronize()
    got, lg = out.cpu().double(), la.cpu().double()
    assert torch.isfinite(got).all() and not torch.isnan(lg).any()
    err, tol = (got - exact).abs(), 2.0 ** -8 * exact.abs() + 2.0 ** -20 * mag
    worst = float((err / tol.clamp_min(1e-300)).max())
    empty = torch.isinf(lse_exact)
    fin = ~empty
    d = (lg[fin] - lse_exact[fin]).abs()
    lworst = float((d / (2.0 ** -19 + 2.0 ** -23 * lse_exact[fin].abs())).max())
    print(f"merge_into2 hd {hd}: largest err / bound {worst:.3f}, lse {lworst:.3f}; all-empty (row, head) pairs {int(empty.sum())}")
    assert bool((err <= tol).all()) and lworst <= 1.0
    assert torch.equal(torch.isinf(lg) & (lg < 0), empty)
    rows = empty.permute(0, 2, 1).unsqueeze(-1).expand(B, Lq, H, hd).reshape(B, Lq, D)
    assert bool(empty.any()) and bool((got[rows] == 0).all()), "an all-empty (row, head) is not zero"
    guard = obuf.cpu().float()
    guard[1:B + 1, 1:Lq + 1, 32:32 + D] = -3.0
    lguard = lbuf.cpu()
    assert bool((guard == -3.0).all()) and bool((lguard[:32] == 123.0).all()) and bool((lguard[32 + B * H * Lq:] == 123.0).all())


@pytest.mark.parametrize("hd", [64, 72, 128])
def test_merge_into2_against_f64(hip_lib, hd):
    _merge_case(hip_lib, hd, seed=hd)


def test_merge_into2_status_codes(hip_lib):
    B, H, Lq, hd = 1, 2, 40, 64
    out = torch.full((B, Lq, H * hd), 3.0, dtype=BF, device=DEV)
    lse = torch.zeros(B, H, Lq, device=DEV)
    o = torch.zeros(B, H, 256, hd, device=DEV)
    l = torch.zeros(B, H, 256, device=DEV)
    st = torch.cuda.current_stream().cuda_stream

    def call(out_=out.data_ptr(), obs=out.stride(0), ors=out.stride(1), lse_=lse.data_ptr(), ob=o.data_ptr(), lb=l.data_ptr(), oc=o.data_ptr(),
             lc=l.data_ptr(), hd_=hd, Lq_=Lq):
        return hip_lib.lib.osk_attention_merge_into2_bf16(out_, obs, ors, lse_, ob, lb, oc, lc, B, H, Lq_, hd_, st)

    EINVAL = -1
    assert call(out_=None) == EINVAL and call(lse_=None) == EINVAL and call(oc=None) == EINVAL and call(lc=None) == EINVAL
    assert call(out_=out.data_ptr() + 2) == EINVAL and call(ors=H * hd + 4) == EINVAL and call(ors=H * hd - 8) == EINVAL
    assert call(oc=o.data_ptr() + 4) == EINVAL and call(lc=l.data_ptr() + 2) == EINVAL and call(Lq_=0) == EINVAL
    assert call(hd_=32) == hip_lib.OSK_EUNSUPPORTED and call(hd_=96) == EINVAL          # (96: the row stride is short of H * hd)
    torch.cuda.synchronize()
    assert bool((out == 3.0).all())


# ----------------------------------------------------------------------------- 2. the entry vs f64
@pytest.mark.parametrize("kind,hd,fast", MODES, ids=[f"{k}-hd{h}{'-FAST' if f else ''}" for k, h, f in MODES])
def test_anchor_entry_vs_f64(hip_lib, kind, hd, fast):
    from open_sora_amd.mmdit import attention_window_bounds

    assert attention_window_bounds(64, 576, 96, 1, 0) == (192, 0) and attention_window_bounds(64, 576, 96, 0, 1) == (64, 128)
    worst = 0.0
    cases = [("g1", a, w, sl) for a, w, sl in G1_CASES] + [("g2", (1, 1), 0, False), ("g2", (1, 1), 1, True)]
    prepared = {}
    for geom, anchors, Wf, sliced in cases:
        q, k, v, sb, n_prefix, n_suffix, t, ref = _case(kind, hd, geom, anchors, Wf, sliced)
        if geom not in prepared:
            prepared[geom] = _prepare(hip_lib, k, v, hd, kind)
        kd, vt, kw = prepared[geom]
        out, lse = _run(hip_lib, q.to(DEV), kd, vt, kw, hd, kind, t, n_prefix, n_suffix, sb if fast else 0.0)
        finite = bool(torch.isfinite(out.float()).all() and torch.isfinite(lse).all())
        r = R.ratios(R.heads(out.float(), H_, hd), lse, ref)
        print(f"anchor {kind} hd {hd}{' FAST' if fast else ''} {geom} anchors {anchors} W {Wf} Lq {q.shape[1]} prefix {n_prefix} suffix "
              f"{n_suffix} table {t.tolist()}: finite {finite}  err/tol {r[0]:.3f}  dlse/tol {r[1]:.3f}")
        assert finite
        worst = max(worst, *r)
    assert worst <= 1.0, worst


# ----------------------------------------------------------------------------- 3. the mask, exactly
@pytest.mark.parametrize("kind,hd,fast", [("bf16", 64, False), ("bf16", 72, True), ("pv8", 72, False), ("qk8", 128, False)])
def test_part_indicator_values_show_the_mask_exactly(hip_lib, kind, hd, fast):
    """V[key, d] = 1 where key lies in body tile d (d < 8), V[key, 9] = 1 for a prefix key, V[key, 10] = 1 for a suffix key: exact in
    bf16 and (scale 1 / 448) in e4m3, so out[row, d] is the share of the row's softmax mass on that part and a tile the row must not
    see contributes no term at all -- exactly 0.  Scores below 1 log2 unit: a visible part's share is within a few percent of the
    f64 share, and 'at least half' cannot fail for any reason but the mask."""
    from open_sora_amd.mmdit import attention_window_bounds, attention_window_table

    L_txt, N, T = GEOMS["g1"]
    L = L_txt + N * T
    g = torch.Generator().manual_seed(17 * hd)
    k = torch.randn(B_, L, H_ * hd, generator=g).to(BF)
    q = torch.randn(B_, L, H_ * hd, generator=g)
    kn = k.float().reshape(B_, L, H_, hd).norm(dim=-1).max()
    q = (q * (0.9 / float(q.reshape(B_, L, H_, hd).norm(dim=-1).max() * kn))).to(BF)
    s = R.heads(q.float(), H_, hd).double() @ R.heads(k.float(), H_, hd).double().transpose(-1, -2)
    assert float(s.abs().max()) < 1.0
    for anchors in ((1, 0), (0, 1), (1, 1)):
        n_prefix, n_suffix = attention_window_bounds(L_txt, N * T, N, *anchors)
        s0 = L - n_suffix
        v = torch.zeros(B_, L, H_, hd)
        v[:, :n_prefix, :, 9] = 1.0
        v[:, s0:, :, 10] = 1.0
        for j in range((s0 - n_prefix) // 64 + (1 if (s0 - n_prefix) % 64 else 0)):
            v[:, n_prefix + 64 * j: min(n_prefix + 64 * (j + 1), s0), :, j] = 1.0
        v = v.reshape(B_, L, H_ * hd).to(BF)
        kd, vt, kw = _prepare(hip_lib, k, v, hd, kind)
        for Wf in (0, 1):
            t = attention_window_table(L_txt, N * T, N, Wf, anchor_head=anchors[0], anchor_tail=anchors[1])
            out, _ = _run(hip_lib, q.to(DEV), kd, vt, kw, hd, kind, t, n_prefix, n_suffix, 1.0 if fast else 0.0, lse=False)
            o = R.heads(out.float(), H_, hd).double()
            lo = 1.0
            for i, (first, n) in enumerate(t.tolist()):
                rows = slice(256 * i, min(256 * (i + 1), L))
                pre, run, suf = A.anchor_key_sets(n_prefix, n_suffix, L, first, n)
                keys = torch.cat([pre, run, suf])
                p = torch.softmax(s[:, :, rows][..., keys] * R.LN2, -1)
                inside = [9] + list(range(first, first + n)) + ([10] if n_suffix else [])
                outside = [d for d in range(hd) if d not in inside]
                stray = o[:, :, rows][..., outside].abs().max().item()
                print(f"indicator {kind} hd {hd} anchors {anchors} W {Wf} block {i} ({first}, {n}): largest value outside the key set {stray:.3e}")
                assert stray == 0.0, (anchors, Wf, i, stray)
                for d in inside:
                    sel = keys < n_prefix if d == 9 else keys >= s0 if d == 10 else (keys >= n_prefix + 64 * d) & (keys < min(n_prefix + 64 * (d + 1), s0))
                    lo = min(lo, (o[:, :, rows, d] / p[..., sel].sum(-1)).min().item())
            print(f"indicator {kind} hd {hd} anchors {anchors} W {Wf}: smallest (kernel mass / f64 mass) inside the key sets {lo:.3f}")
            assert lo >= 0.5, (anchors, Wf, lo)


# ----------------------------------------------------------------------------- 4. no suffix: the window entries, bit for bit
@pytest.mark.parametrize("kind,hd,fast", [("bf16", 64, False), ("bf16", 72, True), ("pv8", 72, False), ("qk8", 128, False)])
def test_without_a_suffix_the_entry_is_the_window_entry_bit_for_bit(hip_lib, kind, hd, fast):
    from open_sora_amd.mmdit import attention_window_table

    L_txt, N, T = 64, 83, 7                                               # 645 keys: a ragged last tile
    L = L_txt + N * T
    q, k, v, sb = _operands(hd, L)
    kd, vt, kw = _prepare(hip_lib, k, v, hd, kind)
    qd = q.to(DEV)
    for n_prefix in (64, 192, 0):
        t = attention_window_table(n_prefix, L - n_prefix, 1, 100)[:3].contiguous()     # three query blocks
        t[1] = torch.tensor([2, 3])
        got, gl = _run(hip_lib, qd, kd, vt, kw, hd, kind, t, n_prefix, 0, sb if fast else 0.0)
        want, wl = torch.full_like(qd, float("nan")), torch.full((B_, H_, L), float("nan"), device=DEV)
        if kind == "bf16":
            hip_lib.attention_fwd_window(qd, kd, vt, want, H_, hd, hd ** -0.5, n_prefix=n_prefix, windows=t, lse=wl, q_prescaled=True,
                                         score_bound=sb if fast else 0.0)
        else:
            hip_lib.attention_fwd_window_fp8(qd, kd, kw["k_scale"], vt, kw["v_scale"], want, H_, hd, hd ** -0.5, n_prefix=n_prefix, windows=t,
                                             mode=kind, lse=wl, q_prescaled=True, Lk=L)
        torch.cuda.synchronize()
        assert torch.isfinite(got.float()).all()
        assert torch.equal(got.view(torch.int16), want.cpu().view(torch.int16)) and torch.equal(gl, wl.cpu()), (kind, n_prefix)


# ----------------------------------------------------------------------------- 5. refused arguments
def test_refused_arguments(hip_lib):
    """status codes of the entry, below the binding's own checks: nothing is launched"""
    hd, Lq, Lk = 128, 800, 512
    q = torch.zeros(1, Lq, H_ * hd, dtype=BF, device=DEV)
    k = torch.zeros(1, Lk, H_ * hd, dtype=BF, device=DEV)
    vt = torch.zeros(1, H_, hd, Lk, dtype=BF, device=DEV)
    k8 = torch.zeros(1, H_, Lk, 128, dtype=torch.uint8, device=DEV)
    vt8 = torch.zeros(1, H_, 144, Lk, dtype=torch.uint8, device=DEV)
    vt8[:, :, hd] = 0x38
    sc = torch.ones(2, H_, device=DEV)
    out = torch.full_like(q, 3.0)
    win = torch.tensor([[0, 4]] * 4, dtype=torch.int32, device=DEV)
    ws = hip_lib.attention_window_anchor_workspace(1, H_, Lq, hd, DEV)
    small = hip_lib.attention_window_workspace_bytes(1, H_, Lq, hd)        # one partial set: not enough for prefix AND suffix
    EINVAL, EUNSUP = -1, hip_lib.OSK_EUNSUPPORTED
    BF16, PV8, QK8 = 0, hip_lib.ATTN_MODES["pv8"], hip_lib.ATTN_MODES["qk8"]

    def call(mode=BF16, n_prefix=64, n_suffix=128, n_windows=4, table=win.data_ptr(), workspace=ws.data_ptr(), ws_bytes=ws.numel(), hd_=hd,
             bound=0.0, v_scale=sc[1].data_ptr(), k_scale=sc[0].data_ptr(), out_=out.data_ptr()):
        kt = k8 if mode == QK8 else k
        v_ = vt if mode == BF16 else vt8
        return hip_lib.lib.osk_attention_fwd_window_anchor_bf16(
            q.data_ptr(), q.stride(0), q.stride(1), kt.data_ptr(), kt.stride(0), 128 if mode == QK8 else kt.stride(1), k_scale, v_.data_ptr(),
            v_scale, out_, out.stride(0), out.stride(1), None, 1, H_, Lq, Lk, n_prefix, n_suffix, hd_, 0.125, 1, 0, bound, mode, table,
            n_windows, workspace, ws_bytes, torch.cuda.current_stream().cuda_stream)

    for mode in (BF16, PV8, QK8):
        # the suffix: negative, Lk - n_suffix no multiple of 64, reaching into (or meeting) the prefix
        assert call(mode, n_suffix=-64) == EINVAL and call(mode, n_suffix=100) == EINVAL and call(mode, n_suffix=160) == EINVAL
        assert call(mode, n_prefix=256, n_suffix=320) == EINVAL and call(mode, n_prefix=256, n_suffix=256) == EINVAL
        # the window entries' list
        assert call(mode, n_windows=3) == EINVAL and call(mode, table=None) == EINVAL and call(mode, table=win.data_ptr() + 2) == EINVAL
        assert call(mode, n_prefix=32) == EINVAL and call(mode, n_prefix=Lk) == EINVAL and call(mode, n_prefix=-64) == EINVAL
        assert call(mode, workspace=None, ws_bytes=0) == EINVAL and call(mode, ws_bytes=small) == EINVAL
        assert call(mode, n_prefix=0, workspace=None, ws_bytes=0) == EINVAL and call(mode, out_=out.data_ptr() + 2) == EINVAL
        assert call(mode, hd_=96) == EUNSUP
    assert call(3) == EINVAL and call(-1) == EINVAL
    assert call(BF16, bound=-1.0) == EINVAL and call(BF16, bound=float("nan")) == EINVAL
    assert call(PV8, v_scale=None) == EINVAL and call(QK8, k_scale=None) == EINVAL and call(QK8, hd_=72) == EUNSUP and call(PV8, hd_=64) == EUNSUP
    torch.cuda.synchronize()
    assert bool((out == 3.0).all())
    # good calls: zero K and V -- uniform probabilities over zero values, every output exactly 0 where it was 3.0; one partial set is
    # enough where only one end is anchored
    for good in (dict(mode=BF16), dict(mode=PV8, k_scale=None), dict(mode=QK8), dict(mode=BF16, n_prefix=0, ws_bytes=small),
                 dict(mode=BF16, n_suffix=0, ws_bytes=small), dict(mode=BF16, v_scale=None, k_scale=None)):
        out.fill_(3.0)
        assert call(**good) == 0, good
        torch.cuda.synchronize()
        assert bool((out == 0.0).all()), good


# ----------------------------------------------------------------------------- 6. capture
def test_anchor_entry_replays_from_a_graph(hip_lib):
    kind, hd = "bf16", 72
    q, k, v, sb, n_prefix, n_suffix, t, _ = _case(kind, hd, "g1", (1, 1), 0, False)
    L = k.shape[1]
    qd, kd, vd = (torch.empty_like(x, device=DEV) for x in (q, k, v))
    vt = torch.zeros(B_, H_, hd, (L + 63) // 64 * 64, dtype=BF, device=DEV)
    out = torch.empty_like(qd)
    ws = torch.empty(hip_lib.attention_window_anchor_workspace_bytes(B_, H_, L, hd), dtype=torch.uint8, device=DEV)

    def fill(flip):
        src_k, src_v = (v, k) if flip else (k, v)
        kd.copy_(src_k.to(DEV)), vd.copy_(src_v.to(DEV)), qd.copy_(q.to(DEV))

    def run():
        hip_lib.v_transpose(vd, vt, H_, hd)
        hip_lib.attention_fwd_window_anchor(qd, kd, vt, out, H_, hd, hd ** -0.5, n_prefix=n_prefix, n_suffix=n_suffix, windows=t, q_prescaled=True,
                                            workspace=ws)

    fill(False)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run()                                                  # side-stream warm-up; also uploads the table outside the capture
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run()
    fill(True)
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    replayed = out.clone()
    out.zero_()
    run()
    torch.cuda.synchronize()
    assert bool(replayed.float().abs().sum() > 0) and torch.isfinite(replayed.float()).all() and torch.equal(replayed, out)


# ----------------------------------------------------------------------------- 7. the model
_T, _h, _w, _LT = 6, 8, 12, 64
_N = _h * _w


def test_anchors_at_the_model_level(hip_lib):
    """64 text + 6 frames x 96 tokens.  Anchors (3, 2) with W = 6 (full tables) leave one frame -- and every query still sees every
    key: the forward agrees with the window off to 2^-7, the bound the window tests hold a full-table forward to.  At W = 0 the
    anchors (1, 1) move the forward."""
    cfg, model = _gpu_model("hd72_eager_split")
    inp = torch_inputs(cfg, 1, _T, _h, _w, _LT, dtype=BF, device="cuda:0")
    n_blocks = cfg["depth"] + cfg["depth_single_blocks"]
    with torch.inference_mode():
        off = model(**inp).float().cpu()
        with _Counting(hip_lib, ["attention_fwd_window_anchor", "attention_fwd_window", "attention_fwd"]) as cnt:
            wide = model.set_attention_window(_T, _N, anchors=(3, 2))(**inp).float().cpu()
        names = [c[0] for c in cnt.calls]
        rep = model.attention_report()["attention_window"]
        narrow = model.set_attention_window(0, _N)(**inp).float().cpu()
        anchored = model.set_attention_window(0, _N, anchors=(1, 1))(**inp).float().cpu()
        with _Counting(hip_lib, ["attention_fwd_window_anchor", "attention_fwd_window"]) as cnt0:
            again = model.set_attention_window(0, _N, anchors=(0, 0))(**inp).float().cpu()
    torch.cuda.synchronize()
    assert names == ["attention_fwd_window_anchor"] * n_blocks, set(names)
    assert {c[0] for c in cnt0.calls} == {"attention_fwd_window"} and torch.equal(again, narrow)
    assert rep["anchors"] == (3, 2) and rep["visited_tile_fraction"] == pytest.approx(1.0)
    e, moved, sep = rel_l2(wide, off), rel_l2(anchored, narrow), rel_l2(narrow, off)
    print(f"model: anchors (3, 2) + full tables vs window off relL2 {e:.3e}; W = 0 anchors (1, 1) vs none {moved:.3e}; W = 0 vs off {sep:.3e}")
    assert torch.isfinite(wide).all() and torch.isfinite(anchored).all()
    assert e <= 2.0 ** -7 and moved > 0 and not torch.equal(anchored, narrow)


SPLITS = [(2, "allgather", "hd72_eager_split", {}, (1, 6, 8, 16, 256)), (2, "ulysses", "hd72_eager_split", {}, (1, 6, 8, 16, 256)),
          (3, "allgather", "hd72_eager_split", {}, (1, _T, _h, _w, _LT)),
          (3, "ulysses", "hd128_liger_split", dict(hidden_size=384, num_heads=3), (1, _T, _h, _w, _LT))]


@pytest.mark.parametrize("P,mode,name,over,geom", SPLITS, ids=[f"P{p}-{m}-{n.split('_')[0]}" for p, m, n, _, _ in SPLITS])
def test_sharded_anchored_forward_is_the_single_device_one(hip_lib, P, mode, name, over, geom):
    """P = 2 aligned (256 + 6 x 128 = 1024 rows: a rank's 256-row blocks are the single-device blocks) and P = 3 ragged (640 rows:
    214, 214, 212 -- blocks that are not the single-device blocks, so W = T: full tables, the anchors still in force), anchors (1, 1),
    ranks as threads.  Bound: the 2^-7 the suite holds a sharded forward to against the single process."""
    cfg, model = _gpu_model(name, **over)
    B, T, h, w, Lt = geom
    inp = torch_inputs(cfg, B, T, h, w, Lt, dtype=BF, device="cuda:0")
    Wf = 1 if P == 2 else T
    model.set_attention_window(Wf, h * w, anchors=(1, 1))
    with torch.inference_mode():
        single = model(**inp).float().cpu()
    torch.cuda.synchronize()
    with _Counting(hip_lib, ["kv_join", "attention_fwd_window_anchor", "attention_fwd_window", "attention_fwd", "attention_fwd_ragged"]) as cnt:
        res = _ranks_forward(model, inp, P, mode, True, n_fwd=1)
    names = {c[0] for c in cnt.calls}
    assert names == {"kv_join", "attention_fwd_window_anchor"}, names
    for outs, _ in res:
        assert torch.equal(outs[0], res[0][0][0])
    e = rel_l2(res[0][0][0], single)
    print(f"P = {P} {mode} {name} anchors (1, 1) W {Wf}: relL2 sharded vs single-device anchored {e:.3e}")
    assert torch.isfinite(res[0][0][0]).all() and e <= 2.0 ** -7, e
