"""CPU: seqpar.enable(..., kv_chunks=S) -- the K / V^T all-gather cut into S key slices, one attention launch per slice, one
osk_attention_merge_bf16 launch -- with P ranks as threads over tests/local_transport.py (and once over gloo) and the CPU
statements of the kernels (tests/cpu_ops.py + tests/cpu_ops_sp_chunked.py): the chunked step against kv_chunks=1, the
effective-S rule, the unchanged call sequence at kv_chunks=1, the modes that ignore the setting, and the C entry's declaration
and argument checks.  The kernels: tests/test_gpu_attention_merge.py, tests/test_gpu_seqpar_chunked.py."""
import copy
import os
import socket
import threading

import pytest
import torch
import torch.multiprocessing as mp

from oracle import configs
from tests.cpu_ops_sp_chunked import Ops, attention_merge, attention_merge_f64
from tests.local_transport import LocalTransport, LocalWorld, run_ranks
from tests.util import rel_l2, torch_inputs, torch_params

BF = torch.bfloat16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture()
def ops_mmdit(hip_lib):
    from open_sora_amd import mmdit

    ops = Ops()
    mmdit.set_ops_for_testing(ops)
    yield mmdit, ops
    mmdit.set_ops_for_testing(hip_lib)


def _cfg72():
    return dict(configs.GOLDEN["hd72_eager_split"][0], depth=1, depth_single_blocks=1)


def _model(mmdit, cfg):
    model = mmdit.Flux(device_map="cpu", torch_dtype=BF, **cfg)
    model.load_state_dict(torch_params(cfg, dtype=BF), strict=True)
    return model


def _run_sp(ops, model, inp, P, mode="allgather", **enable_kw):
    """-> per rank (prediction, the rank's recorded op calls, its SeqPar)"""
    from open_sora_amd import seqpar

    def rank_fn(rank, world):
        m = copy.copy(model)
        m.forward = m.forward_ckpt
        object.__setattr__(m, "_osk_ws_cache", {})
        sp = seqpar.enable(m, mode=mode, transport=LocalTransport(world, rank, "cpu"), **enable_kw)
        with torch.inference_mode():
            out = m(**inp).float().clone()
        return out, threading.get_ident(), sp

    ops.calls.clear()
    res = run_ranks(P, rank_fn, "cpu")
    return [(out, list(ops.calls.get(ident, [])), sp) for out, ident, sp in res]


def _names(calls):
    return [c[0] for c in calls]


def _kw(call):
    return dict(call[2])


def _exchange_calls(calls, D):
    """the recorded calls of the K / V exchange and the attention (the model's own copy_rows glue has other widths than D)"""
    return [c for c in calls if c[0] in ("v_transpose", "attention_fwd", "attention_merge") or (c[0] == "copy_rows" and c[1][0][-1] == D)]


# (P, (B, T, h, w, L_txt)): 12 rows per rank -- 2, 3 and 4 all divide -- with rank 0 holding the text rows and some image rows
GEOMS = {2: (2, 2, 3, 3, 6), 4: (1, 2, 3, 7, 6)}


@pytest.mark.parametrize("S", [2, 3, 4])
@pytest.mark.parametrize("P", [2, 4])
def test_chunked_gather_matches_the_single_gather(ops_mmdit, P, S):
    """kv_chunks = S against kv_chunks = 1 on the same ranks: S copies / transposes / launches per block, one merge, slice by slice;
    the results differ by the bf16 rounding of the S partials under convex weights (each within 2^-9 of its value, so the merged row
    within 2^-9 of its magnitude before its own rounding): the 2^-7 bound the suite holds a sharded forward to against the single
    process (tests/test_seqpar_gloo.py), and the parity rule against the f32 oracle."""
    from oracle import mmdit_oracle as O

    mmdit, ops = ops_mmdit
    cfg = _cfg72()
    H, hd = cfg["num_heads"], cfg["hidden_size"] // cfg["num_heads"]
    geom = GEOMS[P]
    B, Lloc = geom[0], (geom[4] + geom[1] * geom[2] * geom[3]) // P
    assert Lloc == 12
    model = _model(mmdit, cfg)
    inp = torch_inputs(cfg, *geom, dtype=BF)
    n_blocks = cfg["depth"] + cfg["depth_single_blocks"]
    one = _run_sp(ops, model, inp, P, kv_chunks=1)
    res = _run_sp(ops, model, inp, P, kv_chunks=S)
    Lc = Lloc // S
    per_block = (["copy_rows", "v_transpose"] * S) + ["attention_fwd"] * S + ["attention_merge"]
    for out, calls, sp in res:
        assert sp.kv_chunks == S and sp.kv_chunks_for(Lloc) == S
        assert torch.equal(out, res[0][0])                                   # every rank returns the same prediction
        mine = _exchange_calls(calls, H * hd)
        assert _names(mine) == per_block * n_blocks, _names(mine)
        for c in mine:
            if c[0] == "attention_fwd":
                kw = _kw(c)
                assert kw["n_seg"] == P and kw["seg_len"] == Lc and kw["q_prescaled"] is True, kw
                (q, k0, vt, part), lse = c[1], dict(c[3])["lse"]
                assert q == (B, Lloc, H * hd) and k0 == (B, Lc, H * hd) and part == q and lse == (B, H, Lloc), c[1]
                assert vt == (P, B, H, hd, 64), vt
            if c[0] == "attention_merge":
                assert c[1] == ((S, B, Lloc, H * hd), (S, B, H, Lloc), (B, Lloc, H * hd)), c[1]
    err = rel_l2(res[0][0], one[0][0])
    with torch.inference_mode():
        truth = O.forward(torch_params(cfg), cfg, **torch_inputs(cfg, *geom))
        ref_bf16 = O.forward(torch_params(cfg, dtype=BF), cfg, **torch_inputs(cfg, *geom, dtype=BF))
    e_ref, e1, eS = rel_l2(ref_bf16.float(), truth), rel_l2(one[0][0], truth), rel_l2(res[0][0], truth)
    print(f"P = {P} S = {S}: relL2 chunked vs single gather {err:.3e}; vs oracle: S=1 {e1:.3e}, S={S} {eS:.3e}, bf16 reference {e_ref:.3e}")
    assert err <= 2.0 ** -7, err
    assert eS <= max(1.5 * e_ref, 2.0 ** -8), (eS, e_ref)


def test_effective_chunk_count_is_the_largest_divisor():
    from open_sora_amd import seqpar

    tp = LocalTransport(LocalWorld(2), 0, "cpu")
    mk = lambda n: seqpar.SeqPar(transport=tp, mode="allgather", kv_chunks=n)
    assert mk(4).kv_chunks_for(96) == 4
    assert mk(5).kv_chunks_for(96) == 4            # 5 does not divide 96: the next smaller count that does
    assert mk(7).kv_chunks_for(96) == 6
    assert mk(8).kv_chunks_for(97) == 1            # a prime row count: one gather
    assert mk(8).kv_chunks_for(23014) == 2 and mk(8).kv_chunks_for(28864) == 8      # the long-sequence rank shapes
    assert mk(4).kv_chunks_for(3) == 3 and mk(1).kv_chunks_for(96) == 1
    for bad in (0, 9, -1):
        with pytest.raises(ValueError):
            mk(bad)


def test_default_and_environment_variable(monkeypatch):
    from open_sora_amd import seqpar

    tp = LocalTransport(LocalWorld(2), 0, "cpu")
    monkeypatch.delenv("OSK_SP_KV_CHUNKS", raising=False)
    assert seqpar.SeqPar(transport=tp).kv_chunks == 1
    monkeypatch.setenv("OSK_SP_KV_CHUNKS", "4")
    assert seqpar.SeqPar(transport=tp).kv_chunks == 4
    assert seqpar.SeqPar(transport=tp, kv_chunks=2).kv_chunks == 2           # the argument wins
    monkeypatch.setenv("OSK_SP_KV_CHUNKS", "12")
    with pytest.raises(ValueError):
        seqpar.SeqPar(transport=tp)


def test_one_chunk_issues_the_call_sequence_of_the_single_gather(ops_mmdit, monkeypatch):
    """kv_chunks=1 (and the default) is the code path from before the argument existed: per block one K copy, one V transpose, one
    launch over P segments of all the rank's rows, no lse, no merge -- and a prime row count falls back to it whatever was asked"""
    mmdit, ops = ops_mmdit
    monkeypatch.delenv("OSK_SP_KV_CHUNKS", raising=False)
    cfg = _cfg72()
    model = _model(mmdit, cfg)
    n_blocks = cfg["depth"] + cfg["depth_single_blocks"]
    inp = torch_inputs(cfg, *GEOMS[2], dtype=BF)
    default = _run_sp(ops, model, inp, 2)
    one = _run_sp(ops, model, inp, 2, kv_chunks=1)
    for (o0, c0, _), (o1, c1, _) in zip(default, one):
        assert torch.equal(o0, o1) and c0 == c1
        mine = _exchange_calls(c1, cfg["hidden_size"])
        assert _names(mine) == ["copy_rows", "v_transpose", "attention_fwd"] * n_blocks, _names(mine)
        for c in mine:
            if c[0] == "attention_fwd":
                assert _kw(c)["n_seg"] == 2 and _kw(c)["seg_len"] == 12 and len(c[1]) == 4 and not c[3], c      # q, k, vt, out: no lse
    geom = (1, 2, 3, 3, 4)                                                  # L = 22: 11 rows per rank
    inp11 = torch_inputs(cfg, *geom, dtype=BF)
    a, b = _run_sp(ops, model, inp11, 2, kv_chunks=1), _run_sp(ops, model, inp11, 2, kv_chunks=8)
    assert b[0][2].kv_chunks_for(11) == 1 and torch.equal(a[0][0], b[0][0]) and a[0][1] == b[0][1]


def test_head_exchange_and_fp8_attention_ignore_the_setting(ops_mmdit):
    mmdit, ops = ops_mmdit
    cfg = _cfg72()
    model = _model(mmdit, cfg)
    inp = torch_inputs(cfg, *GEOMS[2], dtype=BF)
    a, b = _run_sp(ops, model, inp, 2, mode="ulysses", kv_chunks=1), _run_sp(ops, model, inp, 2, mode="ulysses", kv_chunks=4)
    for (o0, c0, _), (o1, c1, sp) in zip(a, b):
        assert torch.equal(o0, o1) and c0 == c1 and "attention_merge" not in _names(c1)
        assert sp.kv_chunks_applied(cfg["num_heads"]) == 1
    model.enable_fp8()                                                      # pv8 attention: the reduced e4m3 scale is needed first
    a, b = _run_sp(ops, model, inp, 2, kv_chunks=1), _run_sp(ops, model, inp, 2, kv_chunks=4)
    for (o0, c0, _), (o1, c1, sp) in zip(a, b):
        assert torch.equal(o0, o1) and c0 == c1
        assert "attention_merge" not in _names(c1) and _names(c1).count("attention_fwd_pv8") == 2 and "attention_fwd" not in _names(c1)
        assert sp.kv_chunks_applied(cfg["num_heads"], pv8=True) == 1


def test_local_vt_is_none_with_chunks_and_the_projection_writes_v_token_major(ops_mmdit):
    """the V^T GEMM task writes ONE contiguous slot: with S > 1 local_vt() declines, the projection writes V normally and every
    slice is transposed (B = 4, L = 320: the shape at which kv_chunks=1 takes the V^T task, tests/test_seqpar_threads.py)"""
    from open_sora_amd import seqpar

    mmdit, ops = ops_mmdit
    cfg = _cfg72()
    H, hd = cfg["num_heads"], cfg["hidden_size"] // cfg["num_heads"]
    tp = LocalTransport(LocalWorld(2), 1, "cpu")
    assert seqpar.SeqPar(transport=tp, mode="allgather", kv_chunks=4).local_vt(2, 96, H, hd, "cpu") is None
    assert seqpar.SeqPar(transport=tp, mode="allgather", kv_chunks=4).local_vt(2, 97, H, hd, "cpu") is not None    # effective S = 1
    assert tuple(seqpar.SeqPar(transport=tp, mode="allgather").local_vt(2, 96, H, hd, "cpu").shape) == (2, H, hd, 128)
    model = _model(mmdit, cfg)
    inp = torch_inputs(cfg, 4, 4, 8, 8, 64, dtype=BF)
    one, two = _run_sp(ops, model, inp, 2, kv_chunks=1), _run_sp(ops, model, inp, 2, kv_chunks=2)
    assert "v_transpose" not in _names(one[0][1])                           # the V^T task wrote the gather slot
    for out, calls, _ in two:
        assert _names(calls).count("v_transpose") == 2 * 2 and _names(calls).count("attention_merge") == 2
        assert torch.equal(out, two[0][0])
    assert rel_l2(two[0][0], one[0][0]) <= 2.0 ** -7


def test_attention_report_names_the_chunk_count(ops_mmdit):
    from open_sora_amd import seqpar

    mmdit, ops = ops_mmdit
    cfg = _cfg72()
    model = _model(mmdit, cfg)
    assert model.attention_report()["kv_chunks"] == 1                       # no sequence parallelism
    tp = LocalTransport(LocalWorld(2), 0, "cpu")
    seqpar.enable(model, mode="allgather", transport=tp, kv_chunks=5)
    assert model.attention_report()["kv_chunks"] == 5
    assert model.attention_report(2, 96)["kv_chunks"] == 4 and model.attention_report(2, 97)["kv_chunks"] == 1
    seqpar.enable(model, mode="ulysses", transport=tp, kv_chunks=5)
    assert model.attention_report(2, 96)["kv_chunks"] == 1
    seqpar.enable(model, mode="allgather", transport=tp, kv_chunks=5)
    model.enable_fp8()
    assert model.attention_report(2, 96)["kv_chunks"] == 1
    model.enable_fp8(False)
    assert model.attention_report(2, 96)["kv_chunks"] == 4
    seqpar.disable(model)
    assert model.attention_report(2, 96)["kv_chunks"] == 1


# ----------------------------------------------------------------------------------------------- the merge statement and the C entry
def test_cpu_merge_statement_against_f64():
    g = torch.Generator().manual_seed(3)
    S, B, L, H, hd = 3, 2, 5, 2, 16
    parts = torch.randn(S, B, L, H * hd, generator=g).to(BF)
    lse = torch.randn(S, B, H, L, generator=g) * 3
    lse[1, 0, 0, 2] = float("-inf")
    lse[:, 1, 1, 4] = float("-inf")
    out, lo = torch.empty(B, L, H * hd, dtype=BF), torch.empty(B, H, L)
    attention_merge(parts, lse, out, H, hd, lse_out=lo)
    exact, lse_exact, mag = attention_merge_f64(parts, lse)
    assert torch.isfinite(out.float()).all()
    assert ((out.double() - exact).abs() <= 2.0 ** -8 * exact.abs() + 2.0 ** -20 * mag).all()
    assert (out[1, 4, hd:] == 0).all() and lo[1, 1, 4] == float("-inf")
    fin = torch.isfinite(lse_exact)
    assert torch.equal(fin, torch.isfinite(lo)) and (lo[fin].double() - lse_exact[fin]).abs().max() < 1e-5
    one = torch.empty(B, L, H * hd, dtype=BF)
    attention_merge(parts[:1], torch.full((1, B, H, L), 2.5), one, H, hd)
    assert torch.equal(one, parts[0])                                       # one part: the part itself


def test_declared_in_the_header_and_in_the_binding(hip_lib):
    sig = hip_lib.SIGNATURES["osk_attention_merge_bf16"]
    assert len(sig) == 15 and sig[0] is hip_lib._vp and sig[-1] is hip_lib._vp and sig.count(hip_lib._i32) == 5 and sig.count(hip_lib._i64) == 5
    assert hasattr(hip_lib.lib, "osk_attention_merge_bf16") and callable(hip_lib.attention_merge)
    assert hip_lib.lib.osk_abi_version() == 2
    hdr = open(os.path.join(ROOT, "include", "osk.h")).read()
    assert "int osk_attention_merge_bf16(const void* parts," in hdr and "distributed.py:223-313" in hdr


def test_entry_refuses_bad_arguments_without_a_launch(hip_lib):
    """status < 0 from the argument checks of the C entry, before any HIP call (no GPU here)"""
    f = hip_lib.lib.osk_attention_merge_bf16
    order = ("parts", "ps", "pbs", "prs", "lse", "out", "obs", "ors", "lse_out", "S", "B", "H", "L", "hd")
    ok = dict(parts=0x10000, ps=8192, pbs=4096, prs=256, lse=0x20000, out=0x30000, obs=4096, ors=256, lse_out=None, S=2, B=2, H=2, L=16, hd=128)
    call = lambda **kw: f(*[{**ok, **kw}[n] for n in order], None)
    for bad in (dict(parts=None), dict(lse=None), dict(out=None), dict(S=0), dict(S=9), dict(hd=60), dict(hd=0), dict(parts=0x10008),
                dict(out=0x30004), dict(lse=0x20002), dict(lse_out=0x40001), dict(prs=260), dict(ors=252), dict(ors=128), dict(pbs=4100),
                dict(ps=8196), dict(obs=4100), dict(L=0), dict(B=0), dict(H=0)):
        assert call(**bad) == -1, bad
    assert call(H=520, hd=8, prs=4160, ors=4160) == hip_lib.OSK_EUNSUPPORTED
    assert call(B=65536) == hip_lib.OSK_EUNSUPPORTED


def test_wrapper_checks_before_any_launch(hip_lib, monkeypatch):
    class Refuse:
        def __getattr__(self, name):
            raise RuntimeError("the wrapper reached the library: " + name)

    monkeypatch.setattr(hip_lib, "lib", Refuse())
    S, B, L, H, hd = 2, 2, 9, 2, 64
    parts, lse, out = torch.zeros(S, B, L, H * hd, dtype=BF), torch.zeros(S, B, H, L), torch.zeros(B, L, H * hd, dtype=BF)
    with pytest.raises(AssertionError):
        hip_lib.attention_merge(parts.float(), lse, out, H, hd)
    with pytest.raises(AssertionError):
        hip_lib.attention_merge(parts, lse.permute(0, 1, 3, 2), out, H, hd)                  # [S, B, L, H]
    with pytest.raises(AssertionError):
        hip_lib.attention_merge(parts, lse, out[:, :-1], H, hd)
    with pytest.raises(AssertionError):
        hip_lib.attention_merge(torch.zeros(9, B, L, H * hd, dtype=BF), torch.zeros(9, B, H, L), out, H, hd)
    with pytest.raises(AssertionError):
        hip_lib.attention_merge(parts, lse, torch.zeros(B, L, H * hd + 4, dtype=BF)[:, :, 4:], H, hd)   # row stride % 8, alignment
    with pytest.raises(AssertionError):
        hip_lib.attention_merge(parts, lse, out, H, hd, lse_out=torch.zeros(B, L, H))
    with pytest.raises(RuntimeError, match="reached the library"):
        hip_lib.attention_merge(parts, lse, out, H, hd)


# ----------------------------------------------------------------------------------------------- gloo, world 2
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _gloo_worker(rank, world, port, geom, q):
    import torch.distributed as dist

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ.pop("OSK_SP_KV_CHUNKS", None)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.set_num_threads(2)
        from open_sora_amd import mmdit, seqpar

        ops = Ops()
        mmdit.set_ops_for_testing(ops)
        cfg = _cfg72()
        model = _model(mmdit, cfg)
        inp = torch_inputs(cfg, *geom, dtype=BF)
        outs = []
        with torch.inference_mode():
            for S in (1, 3):
                sp = seqpar.enable(model, mode="allgather", kv_chunks=S)
                assert sp.P == world and model.attention_report()["kv_chunks"] == S
                outs.append(model(**inp).float().clone().numpy())
            seqpar.disable(model)
        merges = sum(1 for calls in ops.calls.values() for c in calls if c[0] == "attention_merge")
        q.put((rank, outs, merges))
    except BaseException:
        import traceback

        q.put((rank, "error", traceback.format_exc()))
        raise
    finally:
        dist.destroy_process_group()


def test_chunked_gather_over_gloo_world_2():
    """DistTransport (torch.distributed collectives on flat views of the slice buffers) instead of the thread transport"""
    world, geom = 2, GEOMS[2]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_gloo_worker, args=(r, world, port, geom, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = []
    for _ in range(world):
        r = q.get(timeout=600)
        if isinstance(r[1], str):
            for p in procs:
                p.kill()
            pytest.fail(f"rank {r[0]} failed:\n{r[2]}")
        res.append(r)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    res.sort(key=lambda r: r[0])
    for rank, (one, three), merges in res:
        assert merges == 2                                                  # one per block, in the S = 3 forward only
        assert (three == res[0][1][1]).all() and (one == res[0][1][0]).all()
        err = rel_l2(torch.from_numpy(three), torch.from_numpy(one))
        print(f"gloo rank {rank}: relL2 kv_chunks=3 vs 1 {err:.3e}")
        assert err <= 2.0 ** -7, err
