"""GPU: sequence parallelism over token counts the rank count does not divide.

1. osk_attention_fwd_ragged_bf16 (launch over the n_seg - 1 full key segments + launch over the shorter last one + in-place merge)
   against fp64 on sampled rows and against the single-launch kernel over the same keys laid out as one segment: head_dim 72 / 128,
   n_seg 2 / 4, Lc 130 / 257, last segment of 1, 63, 64, 65, Lc - 1, Lc keys; bf16 (bounded and general body), pv8 and qk8 operands;
   guard bands around out, lse and the workspace.  Tolerances: those tests/test_gpu_rank_shapes.py and tests/test_gpu_attention_qk8.py
   apply to the same bodies.
2. osk_attention_merge_into_bf16 against fp64.
3. P ranks as threads of this process (tests/local_transport.py) on ragged splits, both exchange modes, bf16 / pv8 / qk8; hipGraph capture
   of the entry and of one rank's whole forward.
4. the divisible case keeps its launches and never takes the ragged entry."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF = torch.bfloat16
F8 = torch.float8_e4m3fn
LOG2E = 1.4426950408889634
GUARD = 0xA5


def _unit_rms(t, H, hd):
    t = t.view(*t.shape[:-1], H, hd)
    return (t * torch.rsqrt(t.pow(2).mean(-1, keepdim=True) + 1e-6)).reshape(*t.shape[:-2], H * hd)


def _own_layout(slot, rows, key_axis=3):
    """the slot as the tensor the transposing / packing kernels write for `rows` keys (what the entry reads for the last segment)"""
    shape = list(slot.shape)
    shape[key_axis] = (rows + 63) // 64 * 64
    n = 1
    for d in shape:
        n *= d
    return slot.reshape(-1)[:n].view(shape)


def _ref_rows(q, keys, vals, rows, H, hd, kvb):
    """fp64 softmax(q k^T) v for sample (batch, row) pairs; q pre-scaled (log2 units); keys / vals [kvb, L, D]"""
    outs, lses = [], []
    for b, r in rows:
        bk = b % kvb
        L = keys.shape[1]
        s2 = q[b, r].double().view(H, 1, hd) @ keys[bk].double().view(L, H, hd).permute(1, 2, 0)
        p_ = torch.softmax(s2 / LOG2E, -1)
        outs.append((p_ @ vals[bk].double().view(L, H, hd).permute(1, 0, 2)).reshape(H * hd))
        lses.append(torch.logsumexp(s2 / LOG2E, -1).reshape(H))
    return torch.stack(outs), torch.stack(lses)


def _guarded(shape, dtype, pad_elems=512):
    """a tensor of `shape` inside a byte-pattern guard band on both sides"""
    n = 1
    for d in shape:
        n *= d
    es = torch.empty((), dtype=dtype).element_size()
    raw = torch.full(((n + 2 * pad_elems) * es,), GUARD, dtype=torch.uint8, device=DEV)
    return raw, raw[pad_elems * es: (pad_elems + n) * es].view(dtype).view(shape), pad_elems * es


def _guards_intact(raw, pad_bytes):
    return bool((raw[:pad_bytes] == GUARD).all()) and bool((raw[-pad_bytes:] == GUARD).all())


RAGGED_CASES = [(mode, hd, n_seg, Lc) for mode, hds in (("bf16", (72, 128)), ("pv8", (128,)), ("qk8", (128,)))
                for hd in hds for n_seg in (2, 4) for Lc in (130, 257)] + [("bf16", 64, 4, 130)]   # head_dim 64: the head_dim-72 loop


@pytest.mark.parametrize("mode,hd,n_seg,Lc", RAGGED_CASES, ids=[f"{m}-hd{h}-seg{n}x{l}" for m, h, n, l in RAGGED_CASES])
def test_ragged_entry_against_fp64_and_single_launch(hip_lib, mode, hd, n_seg, Lc):
    H, Bq, Lq = 2, 2, 300                      # two work units per (batch, head), the second one partial
    kvb_arg = 1 if n_seg == 4 else 0           # n_seg 4: the head-exchange form, query batches share one key set
    kvb = kvb_arg or Bq
    D = H * hd
    g = torch.Generator(device=DEV).manual_seed(17 * n_seg + Lc + hd)
    q = (_unit_rms(torch.randn(Bq, Lq, D, device=DEV, generator=g), H, hd) * (hd ** -0.5 * LOG2E)).to(BF)
    k = _unit_rms(torch.randn(n_seg, kvb, Lc, D, device=DEV, generator=g), H, hd).to(BF)
    v = torch.randn(n_seg, kvb, Lc, D, device=DEV, generator=g).to(BF)
    bound = 1.02 * q.float().view(Bq, Lq, H, hd).norm(dim=-1).amax().item() * k.float().view(n_seg, kvb, Lc, H, hd).norm(dim=-1).amax().item()
    assert bound <= 56.0
    Lp = (Lc + 63) // 64 * 64
    RP = hd if mode == "bf16" else hip_lib.vt8_rows(hd)
    need = hip_lib.lib.osk_attention_ragged_workspace_bytes(Bq, H, Lq, hd)
    ws_raw, ws, ws_pad = _guarded((need,), torch.uint8, 256)
    sample = [(b, r) for b in (0, Bq - 1) for r in (0, 31, 255, 256, Lq - 1)]
    for last in (1, 63, 64, 65, Lc - 1, Lc):
        L = (n_seg - 1) * Lc + last
        keys = torch.cat([k[s_] for s_ in range(n_seg - 1)] + [k[-1][:, :last]], 1).contiguous()     # [kvb, L, D]
        vals = torch.cat([v[s_] for s_ in range(n_seg - 1)] + [v[-1][:, :last]], 1).contiguous()
        k_in = k.clone()
        k_in[-1][:, last:] = 100.0             # rows behind the last segment's keys: never to be used
        k_scale = v_scale = None
        vals_deq = vals
        if mode == "bf16":
            vt = torch.zeros(n_seg, kvb, H, hd, Lp, dtype=BF, device=DEV)
            hip_lib.v_transpose(v[:-1].reshape((n_seg - 1) * kvb, Lc, D), vt[:-1].view((n_seg - 1) * kvb, H, hd, Lp), H, hd)
            hip_lib.v_transpose(v[-1][:, :last], _own_layout(vt[-1], last), H, hd)
            k_op = k_in
        else:
            v_scale = (vals.float().abs().view(kvb, L, H, hd).amax(dim=(1, 3)) / 448.0).contiguous()
            vt = torch.zeros(n_seg, kvb, H, RP, Lp, dtype=torch.uint8, device=DEV)
            for s_ in range(n_seg - 1):
                hip_lib.v_transpose_fp8(v[s_], v_scale, vt[s_], H, hd)
            hip_lib.v_transpose_fp8(v[-1][:, :last], v_scale, _own_layout(vt[-1], last), H, hd)
            s4 = v_scale[:, None, :, None]
            vals_deq = ((vals.float().view(kvb, L, H, hd) / s4).clamp(-448, 448).to(F8).float() * s4).view(kvb, L, D)
            k_op = k_in
            if mode == "qk8":
                k_scale = (keys.float().abs().view(kvb, L, H, hd).amax(dim=(1, 3)) / 448.0).contiguous()
                k_op = torch.zeros(n_seg, *hip_lib.k8_shape(kvb, H, Lc, hd), dtype=torch.uint8, device=DEV)
                for s_ in range(n_seg - 1):
                    hip_lib.k_pack_fp8(k[s_], k_scale, k_op[s_], H, hd)
                hip_lib.k_pack_fp8(k[-1][:, :last], k_scale, _own_layout(k_op[-1], last, 2), H, hd)
        ref, ref_lse = _ref_rows(q, keys, vals, sample, H, hd, kvb)
        ref8, _ = _ref_rows(q, keys, vals_deq, sample, H, hd, kvb)
        if mode == "qk8":   # the kernel's operands from the stated rules (include/osk.h): e4m3 K per (batch, head), e4m3 Q per (row, head)
            sk4 = k_scale[:, None, :, None]
            keys_q = ((keys.float().view(kvb, L, H, hd) / sk4).clamp(-448, 448).to(F8).float() * sk4).view(kvb, L, D)
            qf = q.float().view(Bq, Lq, H, hd)
            amax = qf.abs().amax(-1, keepdim=True)
            sq = torch.where(amax > 0, amax / 448.0, torch.ones_like(amax))
            q_q = ((qf / sq).clamp(-448, 448).to(F8).float() * sq).view(Bq, Lq, D)
            ref_q, ref_q_lse = _ref_rows(q_q, keys_q, vals_deq, sample, H, hd, kvb)
        for sb in ((bound, 0.0) if mode == "bf16" else (0.0,)):
            out_raw, out, opad = _guarded((Bq, Lq, D), BF)
            lse_raw, lse, lpad = _guarded((Bq, H, Lq), torch.float32)
            hip_lib.attention_fwd_ragged(q, k_op[0], vt, out, H, hd, hd ** -0.5, n_seg=n_seg, seg_len=Lc, last_seg_len=last,
                                         k_seg_stride=k_op.stride(0), vt_seg_stride=vt.stride(0), workspace=ws, lse=lse,
                                         q_prescaled=True, kv_batches=kvb_arg, score_bound=sb, k_scale=k_scale, v_scale=v_scale)
            torch.cuda.synchronize()
            what = (mode, hd, n_seg, Lc, last, sb)
            assert _guards_intact(out_raw, opad) and _guards_intact(lse_raw, lpad) and _guards_intact(ws_raw, ws_pad), what
            assert bool(torch.isfinite(out.float()).all()) and bool(torch.isfinite(lse).all()), what
            got = torch.stack([out[b, r].double() for b, r in sample])
            got_lse = torch.stack([lse[b, :, r].double() for b, r in sample])
            d_out, d_lse = (got - ref).abs().max().item(), (got_lse - ref_lse).abs().max().item()
            rel, rel8 = ((got - ref).norm() / ref.norm()).item(), ((got - ref8).norm() / ref8.norm()).item()
            print(f"{what}: |out - f64| {d_out:.3e} rel {rel:.3e} rel(e4m3 V) {rel8:.3e} |lse - f64| {d_lse:.3e}")
            if mode == "bf16":
                assert d_out <= 2.5e-2 and d_lse <= 4e-3, (what, d_out, d_lse)
            elif mode == "pv8":
                assert rel8 <= 4e-2 and rel <= 6e-2 and d_lse <= 7e-2, (what, rel8, rel, d_lse)
            else:       # the three gates of tests/test_gpu_attention_qk8.py::_qk8_case
                r_kq, r_q = ((got - ref_q).norm() / ref_q.norm()).item(), ((ref_q - ref).norm() / ref.norm()).item()
                dq_lse = (got_lse - ref_q_lse).abs().max().item()
                print(f"{what}: rel(out, ref_q) {r_kq:.3e} rel(ref_q, ref) {r_q:.3e} |lse - lse_q| {dq_lse:.3e}")
                assert r_kq <= 4e-2 and dq_lse <= 7e-2 and rel <= r_q + 4e-2 + 1e-3, (what, r_kq, dq_lse, rel, r_q)
            if mode != "bf16":
                # the single launch of the same entry over the same keys packed as ONE segment with the same scales.  Each of the
                # two results is within the gate above (4e-2) of the reference built from the shared e4m3 operands; what differs
                # between them is the e4m3 rounding of P against different reference maxima (per launch and key part), so they can
                # be apart by the sum of the two gates at most (triangle inequality); lse likewise, 2 x 7e-2
                Lp1 = (L + 63) // 64 * 64
                vt1 = torch.zeros(kvb, H, RP, Lp1, dtype=torch.uint8, device=DEV)
                hip_lib.v_transpose_fp8(vals, v_scale, vt1, H, hd)
                one, lse1 = torch.empty(Bq, Lq, D, dtype=BF, device=DEV), torch.empty(Bq, H, Lq, dtype=torch.float32, device=DEV)
                kw1 = dict(lse=lse1, q_prescaled=True, kv_batches=kvb_arg, workspace=hip_lib.attention_workspace(q.device))
                if mode == "pv8":
                    hip_lib.attention_fwd_pv8(q, keys, vt1, v_scale, one, H, hd, hd ** -0.5, **kw1)
                else:
                    k81 = torch.zeros(hip_lib.k8_shape(kvb, H, L, hd), dtype=torch.uint8, device=DEV)
                    hip_lib.k_pack_fp8(keys, k_scale, k81, H, hd)
                    hip_lib.attention_fwd_qk8(q, k81, k_scale, vt1, v_scale, one, H, hd, hd ** -0.5, seg_len=L, **kw1)
                r_pair = ((out.float() - one.float()).norm() / one.float().norm()).item()
                d_pair = (lse - lse1).abs().max().item()
                print(f"{what}: rel(ragged, single launch) {r_pair:.3e} |lse - lse_single| {d_pair:.3e}")
                assert r_pair <= 2 * 4e-2 and d_pair <= 2 * 7e-2, (what, r_pair, d_pair)
                continue
            # the single-launch kernel over the same keys as ONE segment.  Both results carry the kernels' error against the exact
            # one; on top the ragged form rounds launch A's rows to bf16 before the merge rounds again: three half-ulp roundings
            # (2^-9 relative each) between the two, < 2^-7 of the largest value, + 1e-3 for the f32 sums' different order
            vt1 = torch.zeros(kvb, H, hd, (L + 63) // 64 * 64, dtype=BF, device=DEV)
            hip_lib.v_transpose(vals, vt1, H, hd)
            one, lse1 = torch.empty(Bq, Lq, D, dtype=BF, device=DEV), torch.empty(Bq, H, Lq, dtype=torch.float32, device=DEV)
            hip_lib.attention_fwd(q, keys, vt1, one, H, hd, hd ** -0.5, lse=lse1, q_prescaled=True, kv_batches=kvb_arg,
                                  workspace=hip_lib.attention_workspace(q.device), score_bound=sb)
            assert (out.float() - one.float()).abs().max().item() <= 2 ** -7 * one.float().abs().max().item() + 1e-3, what
            assert (lse - lse1).abs().max().item() <= 4e-3, what


def test_ragged_entry_status_conventions(hip_lib):
    """OSK_EINVAL before anything is launched: one segment, an empty or over-long last segment, no workspace, too small a one"""
    H, hd, Lq, Lc = 2, 128, 64, 130
    D = H * hd
    q = torch.zeros(1, Lq, D, dtype=BF, device=DEV)
    k = torch.zeros(2, 1, Lc, D, dtype=BF, device=DEV)
    vt = torch.zeros(2, 1, H, hd, 192, dtype=BF, device=DEV)
    out = torch.zeros(1, Lq, D, dtype=BF, device=DEV)
    ws = torch.empty(hip_lib.lib.osk_attention_ragged_workspace_bytes(1, H, Lq, hd), dtype=torch.uint8, device=DEV)

    def call(n_seg=2, last=5, wsp=ws.data_ptr(), ws_bytes=ws.numel(), mode=0):
        return hip_lib.lib.osk_attention_fwd_ragged_bf16(q.data_ptr(), q.stride(0), q.stride(1), k.data_ptr(), k.stride(0), k.stride(1), k.stride(2),
                                                         None, vt.data_ptr(), vt.stride(0), None, out.data_ptr(), out.stride(0), out.stride(1), None,
                                                         1, H, Lq, n_seg, Lc, last, hd, 1.0, 1, 0, 0.0, mode, wsp, ws_bytes,
                                                         torch.cuda.current_stream().cuda_stream)

    assert call() == 0
    for bad in (dict(n_seg=1), dict(last=0), dict(last=Lc + 1), dict(wsp=None), dict(ws_bytes=1024), dict(mode=3), dict(mode=1)):
        assert call(**bad) == -1, bad
    torch.cuda.synchronize()


@pytest.mark.parametrize("hd", [72, 128])
def test_merge_into_against_fp64(hip_lib, hd):
    """the in-place two-part merge: a side without mass (lse = -inf, its rows holding NaN), both sides equal, both empty, an odd Lq
    behind a full 256-row block; out is a strided view whose neighbouring columns and guard bands must stay as they were.
    Tolerance: f32 sums rounded once to bf16 (2^-9 relative) + f32 noise of the weights."""
    B, H, Lq = 2, 3, 301
    D, Lqp = H * hd, 512
    g = torch.Generator(device=DEV).manual_seed(hd)
    raw, wide, pad = _guarded((B, Lq, D + 16), BF)
    wide.copy_(torch.randn(B, Lq, D + 16, device=DEV, generator=g).to(BF))
    out = wide[:, :, 8: 8 + D]
    side = wide.clone()
    o_a = out.clone()
    lse_raw, lse, lpad = _guarded((B, H, Lq), torch.float32)
    lse.copy_(torch.randn(B, H, Lq, device=DEV, generator=g) * 3 + 5)
    ob_raw, o_b, bpad = _guarded((B, H, Lqp, hd), torch.float32)
    o_b.copy_(torch.randn(B, H, Lqp, hd, device=DEV, generator=g))
    lse_b = torch.randn(B, H, Lqp, device=DEV, generator=g) * 3 + 5
    lse_b[:, :, 0:40] = float("-inf")                  # B without mass ...
    o_b[:, :, 0:40] = float("nan")                     # ... and its rows garbage
    lse[:, :, 40:80] = float("-inf")                   # A without mass
    lse_b[:, :, 80:120] = lse[:, :, 80:120]            # equal
    lse[:, :, 299] = float("-inf")
    lse_b[:, :, 299] = float("-inf")                   # both empty
    la, lb = lse.double().clone(), lse_b[:, :, :Lq].double()
    m = torch.maximum(la, lb)
    m0 = torch.where(torch.isinf(m), torch.zeros_like(m), m)
    wa, wb = torch.exp(la - m0), torch.exp(lb - m0)
    tot = wa + wb
    safe = torch.where(tot > 0, tot, torch.ones_like(tot))
    A = o_a.double().view(B, Lq, H, hd)
    Bp = torch.nan_to_num(o_b[:, :, :Lq].double().permute(0, 2, 1, 3), nan=0.0)
    ref = ((wa / safe).permute(0, 2, 1)[..., None] * A + (wb / safe).permute(0, 2, 1)[..., None] * Bp).reshape(B, Lq, D)
    ref_lse = torch.where(tot > 0, m0 + torch.log(safe), torch.full_like(m, float("-inf")))
    hip_lib.attention_merge_into(out, lse, o_b, lse_b, H, hd)
    torch.cuda.synchronize()
    assert _guards_intact(raw, pad) and _guards_intact(lse_raw, lpad) and _guards_intact(ob_raw, bpad)
    assert torch.equal(wide[:, :, :8], side[:, :, :8]) and torch.equal(wide[:, :, 8 + D:], side[:, :, 8 + D:])
    err = (out.double() - ref).abs()
    assert bool((err <= 2.0 ** -8 * ref.abs() + 1e-6).all()), err.max().item()
    assert torch.equal(out[:, 0:40], o_a[:, 0:40]), "a part without mass must leave the rows as they are"
    assert bool((out[:, 299] == 0).all())
    fin = torch.isfinite(ref_lse)
    assert torch.equal(torch.isfinite(lse), fin)
    assert (lse.double()[fin] - ref_lse[fin]).abs().max().item() <= 2e-5 * 16


def test_ragged_attention_is_hipgraph_capturable(hip_lib):
    """the ragged entry allocates nothing and never synchronises: captured once, replayed on new operands == the eager call"""
    H, hd, n_seg, Lc, last, Lq = 2, 72, 4, 130, 65, 300
    D, Lp = H * hd, 192
    g = torch.Generator(device=DEV).manual_seed(5)
    q = torch.empty(1, Lq, D, dtype=BF, device=DEV)
    k = torch.empty(n_seg, 1, Lc, D, dtype=BF, device=DEV)
    vt = torch.zeros(n_seg, 1, H, hd, Lp, dtype=BF, device=DEV)
    out = torch.empty(1, Lq, D, dtype=BF, device=DEV)
    ws = torch.empty(hip_lib.lib.osk_attention_ragged_workspace_bytes(1, H, Lq, hd), dtype=torch.uint8, device=DEV)

    def fill():
        q.copy_((_unit_rms(torch.randn(1, Lq, D, device=DEV, generator=g), H, hd) * (hd ** -0.5 * LOG2E)).to(BF))
        k.copy_(_unit_rms(torch.randn(n_seg, 1, Lc, D, device=DEV, generator=g), H, hd).to(BF))
        v = torch.randn(n_seg, 1, Lc, D, device=DEV, generator=g).to(BF)
        hip_lib.v_transpose(v[:-1].reshape(n_seg - 1, Lc, D), vt[:-1].view(n_seg - 1, H, hd, Lp), H, hd)
        hip_lib.v_transpose(v[-1][:, :last], _own_layout(vt[-1], last), H, hd)

    def run():
        hip_lib.attention_fwd_ragged(q, k[0], vt, out, H, hd, hd ** -0.5, n_seg=n_seg, seg_len=Lc, last_seg_len=last,
                                     k_seg_stride=k.stride(0), vt_seg_stride=vt.stride(0), workspace=ws, q_prescaled=True, score_bound=40.0)

    fill()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run()
    fill()
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    replayed = out.clone()
    out.zero_()
    run()
    torch.cuda.synchronize()
    assert bool(replayed.float().abs().sum() > 0) and torch.equal(replayed, out)


class _EchoTransport:
    """a rank whose peers echo it (tests/test_gpu_seqpar_chunked.py): every collective runs on the caller's stream with this rank's
    own chunk in every slot -- one thread, one stream, no events from other ranks, which is what a stream capture needs.  Not the
    model's prediction, but the launches, buffers, views and workspace of a real rank of a ragged split."""

    class _Done:
        def wait(self):
            return True

    def __init__(self, P, rank):
        self.P, self.rank = P, rank

    def all_gather(self, out, inp):
        o = out.view(self.P, -1)
        for s in range(self.P):
            if o[s].data_ptr() != inp.data_ptr():
                o[s].copy_(inp.view(-1))
        return self._Done()

    def all_reduce_max(self, t):
        return self._Done()


@pytest.mark.parametrize("rank,fp8", [(0, False), (1, False), (1, True)], ids=["rank0", "last_rank", "last_rank_fp8"])
def test_ragged_block_forward_is_hipgraph_capturable(hip_lib, rank, fp8):
    """one rank's whole forward on a ragged split (P = 2, L = 321: 161 rows on rank 0, 160 on the last rank; all-gather mode) captured
    in a torch.cuda.graph and replayed == the eager forward, bit for bit: the sliced copies into zero-filled slots, the own-layout
    views, the workspace cache, two launches + the merge per block, and the cut of the gathered prediction"""
    import copy

    from open_sora_amd import mmdit, seqpar
    from oracle import configs
    from tests.util import torch_inputs, torch_params

    cfg = configs.GOLDEN["hd72_eager_split"][0]
    m = mmdit.Flux(device_map="cuda:0", torch_dtype=BF, **cfg)
    m.load_state_dict(torch_params(cfg, dtype=BF, device="cuda:0"), strict=True)
    if fp8:
        m.enable_fp8()
    inp = torch_inputs(cfg, 2, 4, 8, 8, 65, dtype=BF, device="cuda:0")
    sp = seqpar.enable(m, mode="allgather", transport=_EchoTransport(2, rank))
    with _Counting(hip_lib, ["attention_fwd_ragged"]) as cnt, torch.inference_mode():
        eager = m(**inp).clone()
        torch.cuda.synchronize()
        assert sp.geom == (161, 160) and eager.shape[1] == 256
        n_blocks = cfg["depth"] + cfg["depth_single_blocks"]
        assert len(cnt.calls) == n_blocks and all(c[1:] == (2, 161, 160) for c in cnt.calls)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            m(**inp)                               # side-stream warm-up, as torch's capture recipe asks
        torch.cuda.current_stream().wait_stream(s)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            res = m(**inp)
        for _ in range(2):
            res.zero_()
            graph.replay()
            torch.cuda.synchronize()
            assert torch.isfinite(res.float()).all() and torch.equal(res, eager), "hipGraph replay differs from the eager forward"


class _Counting:
    """counts the calls of some functions of the kernel table while a test runs (and records their segment arguments)"""

    def __init__(self, lib, names):
        self.lib, self.names, self.calls, self.saved = lib, names, [], {}

    def __enter__(self):
        for n in self.names:
            fn = self.saved[n] = getattr(self.lib, n)
            setattr(self.lib, n, (lambda fn_, n_: lambda *a, **kw: (self.calls.append((n_, kw.get("n_seg"), kw.get("seg_len"), kw.get("last_seg_len"))),
                                                                    fn_(*a, **kw))[1])(fn, n))
        return self

    def __exit__(self, *exc):
        for n, fn in self.saved.items():
            setattr(self.lib, n, fn)


def _ranks_forward(model, inp, P, mode, overlap, n_fwd=2):
    import copy

    from open_sora_amd import seqpar
    from tests.local_transport import LocalTransport, run_ranks

    def rank_fn(rank, world):
        m = copy.copy(model)
        m.forward = m.forward_ckpt
        object.__setattr__(m, "_osk_ws_cache", {})
        sp = seqpar.enable(m, mode=mode, transport=LocalTransport(world, rank, "cuda:0", overlap=overlap))
        with torch.inference_mode():
            outs = [m(**inp).float() for _ in range(n_fwd)]
        torch.cuda.current_stream().synchronize()
        return [o.cpu() for o in outs], sp.geom

    return run_ranks(P, rank_fn, "cuda:0")


SP_RAGGED = [
    (4, "hd72_eager_split", (1, 4, 8, 8, 65)),     # L = 4 * 80 + 1: 81 + 81 + 81 + 78
    (4, "hd72_eager_split", (1, 4, 8, 8, 67)),     # L = 4 * 80 + 3: 81 + 81 + 81 + 80
    (2, "hd128_liger_split", (3, 2, 9, 7, 23)),    # L = 149: 75 + 74, CFG-triple batch
]


@pytest.mark.parametrize("mode", ["allgather", "ulysses"])
@pytest.mark.parametrize("case", SP_RAGGED, ids=lambda c: f"w{c[0]}-{c[1]}-L{c[2][4] + c[2][1] * c[2][2] * c[2][3]}")
def test_ragged_seqpar_ranks_as_threads(hip_lib, case, mode):
    """ragged splits with P ranks as threads on the one GPU: overlapped exchange == serial order bit for bit, the ranks agree, the
    forward repeats, and it equals the single-device forward and the oracle within the bounds of tests/test_gpu_overlap.py"""
    from open_sora_amd import mmdit
    from oracle import configs, mmdit_oracle as O
    from tests.util import rel_l2, torch_inputs, torch_params

    P, name, geom = case
    cfg = configs.GOLDEN[name][0]
    assert cfg["num_heads"] % P == 0
    B, T, h, w, L_txt = geom
    L = L_txt + T * h * w
    dev = "cuda:0"
    model = mmdit.Flux(device_map=dev, torch_dtype=torch.bfloat16, **cfg)
    model.load_state_dict(torch_params(cfg, dtype=torch.bfloat16, device=dev), strict=True)
    inp = torch_inputs(cfg, B, T, h, w, L_txt, dtype=torch.bfloat16, device=dev)
    with torch.inference_mode():
        single = model(**inp).float().cpu()
    torch.cuda.synchronize()
    with _Counting(hip_lib, ["attention_fwd_ragged"]) as cnt:
        serial, over = _ranks_forward(model, inp, P, mode, False), _ranks_forward(model, inp, P, mode, True)
    Lc = -(-L // P)
    n_blocks = cfg["depth"] + cfg["depth_single_blocks"]
    assert len(cnt.calls) == 2 * 2 * P * n_blocks and all(c[1:] == (P, Lc, L - (P - 1) * Lc) for c in cnt.calls), cnt.calls[:3]
    for res in (serial, over):
        for outs, geom_ in res:
            assert geom_ == (Lc, L - (P - 1) * Lc)
            assert outs[0].shape == single.shape and torch.equal(outs[0], outs[1]), "sequence-parallel forward is not repeatable"
            assert torch.equal(outs[0], res[0][0][0]), "ranks disagree on the gathered prediction"
    assert torch.equal(over[0][0][0], serial[0][0][0]), "overlapped exchange differs from the serial order"
    with torch.inference_mode():
        truth = O.forward(torch_params(cfg), cfg, **torch_inputs(cfg, B, T, h, w, L_txt))
        ref_bf16 = O.forward(torch_params(cfg, dtype=torch.bfloat16), cfg, **torch_inputs(cfg, B, T, h, w, L_txt, dtype=torch.bfloat16))
    e_ref, e_sp = rel_l2(ref_bf16.float(), truth), rel_l2(over[0][0][0], truth)
    assert e_sp <= max(1.5 * e_ref, 2.0 ** -8), (e_sp, e_ref)
    assert rel_l2(over[0][0][0], single) <= 2.0 ** -7


@pytest.mark.parametrize("mode", ["allgather", "ulysses"])
@pytest.mark.parametrize("qk8", [False, True], ids=["pv8", "qk8"])
def test_ragged_seqpar_ranks_as_threads_fp8(hip_lib, qk8, mode):
    """the fp8 handles through seqpar on a ragged split (P = 2, L = 149 = 75 + 74, head_dim 128): e4m3 V^T -- and with qk8 e4m3 K -- of
    the last rank written in the layout of its own rows, scales agreed across the ranks; every rank's attention is the ragged entry on
    those operands.  Sharded == single-device fp8 forward within the bound tests/test_gpu_seqpar_qk8.py applies (2e-2); ranks agree.
    B = 1: with fewer than 256 rows per Linear neither the single-device forward nor a rank runs the fp8 GEMMs (gemm_fp8_supported), so
    the two forwards differ through the attention alone.  (At B = 3 the single-device Linears are fp8 and a rank's are bf16: the
    comparison then measures the Linears' e4m3 error, 2.5e-2 at L = 148 -- a divisible length -- and at L = 149 alike.)"""
    from open_sora_amd import mmdit
    from oracle import configs
    from tests.util import rel_l2, torch_inputs, torch_params

    P, name, (_, T, h, w, L_txt) = SP_RAGGED[2]
    B = 1
    cfg = configs.GOLDEN[name][0]
    model = mmdit.Flux(device_map="cuda:0", torch_dtype=BF, **cfg)
    model.load_state_dict(torch_params(cfg, dtype=BF, device="cuda:0"), strict=True)
    model.enable_fp8(qk8=qk8)
    inp = torch_inputs(cfg, B, T, h, w, L_txt, dtype=BF, device="cuda:0")
    with torch.inference_mode():
        single = model(**inp).float().cpu()
    torch.cuda.synchronize()
    saved, seen = hip_lib.attention_fwd_ragged, []

    def spy(*a, **kw):
        seen.append((kw.get("k_scale") is not None, kw.get("v_scale") is not None, kw["seg_len"], kw["last_seg_len"]))
        return saved(*a, **kw)

    hip_lib.attention_fwd_ragged = spy
    try:
        res = _ranks_forward(model, inp, P, mode, True)
    finally:
        hip_lib.attention_fwd_ragged = saved
    n_blocks = cfg["depth"] + cfg["depth_single_blocks"]
    assert len(seen) == 2 * P * n_blocks and all(c == (qk8, True, 75, 74) for c in seen), seen[:3]
    for outs, geom_ in res:
        assert geom_ == (75, 74) and torch.equal(outs[0], outs[1]) and torch.equal(outs[0], res[0][0][0])
    e = rel_l2(res[0][0][0], single)
    print(f"ragged fp8 qk8={qk8} {mode}: relL2 sharded vs single {e:.3e}")
    assert e <= 2e-2, e


@pytest.mark.parametrize("P,name,geom,kernel,body", [
    (4, "hd72_eager_split", (1, 4, 8, 8, 64), "attn_asm72_kernel", "attn_asm72_kernel<general>"),       # 80 keys per segment: 2 tiles
    (2, "hd72_eager_split", (2, 4, 8, 8, 64), "attn_asm72_kernel", "attn_asm72_kernel<FAST>"),          # 160: 3 tiles
    (2, "hd128_liger_split", (3, 2, 9, 7, 22), "attn_asm128_kernel", "attn_asm128_kernel<general>"),    # 74: 2 tiles
], ids=["w4-hd72", "w2-hd72", "w2-hd128"])
def test_divisible_split_keeps_its_launches(hip_lib, P, name, geom, kernel, body):
    """P | L: one osk_attention_fwd_bounded_bf16 launch per block over P segments of L / P keys, the kernel and body names the
    dispatch reported before the ragged entry existed -- and the ragged entry is never called"""
    from open_sora_amd import mmdit
    from oracle import configs
    from tests.util import torch_inputs, torch_params

    cfg = configs.GOLDEN[name][0]
    B, T, h, w, L_txt = geom
    L = L_txt + T * h * w
    assert L % P == 0
    hd = cfg["hidden_size"] // cfg["num_heads"]
    model = mmdit.Flux(device_map="cuda:0", torch_dtype=torch.bfloat16, **cfg)
    model.load_state_dict(torch_params(cfg, dtype=torch.bfloat16, device="cuda:0"), strict=True)
    inp = torch_inputs(cfg, B, T, h, w, L_txt, dtype=torch.bfloat16, device="cuda:0")
    with torch.inference_mode():
        model(**inp)
    torch.cuda.synchronize()
    with _Counting(hip_lib, ["attention_fwd_ragged", "attention_fwd"]) as cnt:
        res = _ranks_forward(model, inp, P, "allgather", True, n_fwd=1)
    n_blocks = cfg["depth"] + cfg["depth_single_blocks"]
    assert all(g_ == (L // P, L // P) for _, g_ in res)
    assert [c[0] for c in cnt.calls].count("attention_fwd_ragged") == 0
    assert len(cnt.calls) == P * n_blocks and all(c == ("attention_fwd", P, L // P, None) for c in cnt.calls), cnt.calls[:3]
    rep = model.attention_report(P, L // P)
    assert "ragged" not in rep
    assert hip_lib.lib.osk_attention_kernel_name(hd, L // P).decode() == kernel
    assert hip_lib.attention_body(hd, P, L // P, 40.0) == body        # the parent's selector: FAST needs >= 3 tiles per segment
    tiles = (L // P + 63) // 64
    for bound in (rep["score_bound_min"], rep["score_bound_max"]):
        want = f"{kernel}<{'FAST' if 0.0 < bound <= 56.0 and tiles >= 3 else 'general'}>"
        assert hip_lib.attention_body(hd, P, L // P, bound) == want and want in rep["bodies"]
    rag = model.attention_report(P, L // P + 1, L // P - P + 1)
    assert rag["kv_chunks"] == 1 and rag["ragged"]["attention_entry_launches"] == 3 and rag["ragged"]["last_seg_len"] == L // P - P + 1
