"""CPU: enable_fp8(qk8=True) under sequence parallelism, P ranks as threads over tests/local_transport.py and the CPU statements
of the kernels (tests/cpu_ops.py + tests/cpu_ops_sp_qk8.py): every rank runs the qk8 attention in both exchange modes, the
reduced [2, B, H] scales agree on every rank, all-gather mode issues exactly ONE reducing collective per block and head-exchange
mode none, and the binding of the new entry checks its arguments before any launch.  The kernels: tests/test_gpu_seqpar_qk8.py."""
import copy
import threading

import pytest
import torch

from oracle import configs
from tests.cpu_ops_sp_qk8 import Ops
from tests.local_transport import LocalTransport, run_ranks
from tests.util import rel_l2, torch_inputs, torch_params

BF = torch.bfloat16


class CountingTransport(LocalTransport):
    """LocalTransport that counts its collectives by kind"""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.n = {"all_reduce_max": 0, "all_gather": 0, "all_to_all": 0}
        self.reduced = []          # shapes of the max-reduced buffers

    def all_reduce_max(self, t):
        self.n["all_reduce_max"] += 1
        assert t.dtype == torch.float32 and t.is_contiguous()
        self.reduced.append(tuple(t.shape))
        return super().all_reduce_max(t)

    def all_gather(self, out, inp):
        self.n["all_gather"] += 1
        return super().all_gather(out, inp)

    def all_to_all(self, out, inp):
        self.n["all_to_all"] += 1
        return super().all_to_all(out, inp)


@pytest.fixture()
def ops_mmdit(hip_lib):
    from open_sora_amd import mmdit

    ops = Ops()
    mmdit.set_ops_for_testing(ops)
    yield mmdit, ops
    mmdit.set_ops_for_testing(hip_lib)


def _model(mmdit, cfg):
    model = mmdit.Flux(device_map="cpu", torch_dtype=BF, **cfg)
    model.load_state_dict(torch_params(cfg, dtype=BF), strict=True)
    return model


def _cfg128(heads):
    """the small head_dim-128 model (tests/test_gpu_fp8.py::test_mmdit_forward_fp8_mode), widened to `heads` heads where the head
    exchange needs them to divide by P"""
    return dict(configs.GOLDEN["hd128_eager_fused"][0], depth=1, depth_single_blocks=1, hidden_size=128 * heads, num_heads=heads)


def _run_sp(mmdit, ops, model, inp, P, mode):
    from open_sora_amd import seqpar

    def rank_fn(rank, world):
        m = copy.copy(model)
        m.forward = m.forward_ckpt
        object.__setattr__(m, "_osk_ws_cache", {})
        tp = CountingTransport(world, rank, "cpu")
        sp = seqpar.enable(m, mode=mode, transport=tp)
        assert sp.P == P and sp.head_parallel(model.num_heads) == (mode == "ulysses")
        with torch.inference_mode():
            return m(**inp).float().clone(), dict(tp.n, reduced=tp.reduced), threading.get_ident()

    ops.qk8_calls.clear()
    ops.pv8_calls.clear()
    return run_ranks(P, rank_fn, "cpu")


# SP against the single-process forward in fp8 mode: the bound tests/test_gpu_seqpar_1gpu.py applies to its fp8 case.  The scales
# and the K bytes are the single device's by construction; what differs is the row chunking of the fp8 Linears' dynamic activation
# scales' inputs (bf16 roundings of GEMMs over other row counts), which e4m3 rounding can turn into a flipped code here and there.
SP_VS_SINGLE = 2e-2


@pytest.mark.parametrize("mode", ["allgather", "ulysses"])
@pytest.mark.parametrize("P,heads,geom", [(2, 2, (2, 2, 2, 4, 4)), (4, 4, (1, 2, 3, 4, 4))], ids=["w2", "w4"])
def test_qk8_runs_on_every_rank_under_sequence_parallelism(ops_mmdit, mode, P, heads, geom):
    mmdit, ops = ops_mmdit
    cfg = _cfg128(heads)
    n_blocks = cfg["depth"] + cfg["depth_single_blocks"]
    model = _model(mmdit, cfg).enable_fp8(qk8=True)
    inp = torch_inputs(cfg, *geom, dtype=BF)
    B = geom[0]
    with torch.inference_mode():
        single = model(**inp).float().clone()
    assert len(ops.qk8_calls[threading.get_ident()]) == n_blocks and not ops.pv8_calls

    res = _run_sp(mmdit, ops, model, inp, P, mode)
    assert not ops.pv8_calls, ops.pv8_calls                                       # no rank fell back to the pv8 attention
    per_rank = [ops.qk8_calls.get(ident, []) for _, _, ident in res]
    assert [len(c) for c in per_rank] == [n_blocks] * P
    for out, n, _ in res:
        assert torch.equal(out, res[0][0])
        # ONE reducing collective per block in all-gather mode (K's and V's scales in one [2, B, H] buffer), none in head-exchange mode
        assert n["all_reduce_max"] == (n_blocks if mode == "allgather" else 0), n
        assert n["reduced"] == ([(2, B, heads)] * n_blocks if mode == "allgather" else []), n
        if mode == "allgather":
            assert n["all_to_all"] == 0 and n["all_gather"] == 2 * n_blocks + 1, n      # K and V^T per block, the prediction once
        else:
            assert n["all_to_all"] == 4 * n_blocks and n["all_gather"] == 1, n          # k, v, q, o per block
    if mode == "allgather":      # every rank holds the scales of ALL heads: the same on every rank, block by block
        for blk in range(n_blocks):
            sk0, sv0 = per_rank[0][blk]
            assert sk0.shape == (B, heads) and sv0.shape == (B, heads)
            for r in range(1, P):
                assert torch.equal(per_rank[r][blk][0], sk0) and torch.equal(per_rank[r][blk][1], sv0)
    err = rel_l2(res[0][0], single)
    print(f"P = {P} {mode}: relL2 SP vs single (CPU statements, qk8) {err:.3e}")
    assert err <= SP_VS_SINGLE, err


@pytest.mark.parametrize("mode", ["allgather", "ulysses"])
def test_head_dim_72_and_plain_fp8_keep_the_pv8_exchange(ops_mmdit, mode):
    mmdit, ops = ops_mmdit
    cfg72 = dict(configs.GOLDEN["hd72_eager_split"][0], depth=1, depth_single_blocks=1)
    m72 = _model(mmdit, cfg72).enable_fp8(qk8=True)
    inp72 = torch_inputs(cfg72, 2, 2, 2, 4, 4, dtype=BF)
    res = _run_sp(mmdit, ops, m72, inp72, 2, mode)
    assert not ops.qk8_calls and sorted(ops.pv8_calls.values()) == [2, 2]
    with_flag = res[0][0]
    res = _run_sp(mmdit, ops, m72.enable_fp8(), inp72, 2, mode)
    assert torch.equal(res[0][0], with_flag)                                       # head_dim 72: the flag changes nothing

    cfg = _cfg128(2)
    model = _model(mmdit, cfg).enable_fp8()                                        # qk8 not asked for
    res = _run_sp(mmdit, ops, model, torch_inputs(cfg, 2, 2, 2, 4, 4, dtype=BF), 2, mode)
    assert not ops.qk8_calls and sorted(ops.pv8_calls.values()) == [2, 2]
    for _, n, _ in res:
        assert n["all_reduce_max"] == (2 if mode == "allgather" else 0)


def test_an_sp_object_without_the_argument_keeps_working(ops_mmdit):
    """mmdit passes qk8 only to an sp object that declares it (kv_qk8), the way local_vt is looked up before it is used"""
    from open_sora_amd import seqpar

    mmdit, ops = ops_mmdit

    class OldSeqPar(seqpar.SeqPar):
        kv_qk8 = False

        def gather_kv_start(self, ws, k, v, H, hd, pv8=False, vt_ready=False):
            return super().gather_kv_start(ws, k, v, H, hd, pv8, vt_ready=vt_ready)

    cfg = _cfg128(2)
    model = _model(mmdit, cfg).enable_fp8(qk8=True)
    inp = torch_inputs(cfg, 2, 2, 2, 4, 4, dtype=BF)

    def rank_fn(rank, world):
        m = copy.copy(model)
        m.forward = m.forward_ckpt
        object.__setattr__(m, "_osk_ws_cache", {})
        m._sp = OldSeqPar(mode="allgather", transport=LocalTransport(world, rank, "cpu"))
        with torch.inference_mode():
            return m(**inp).float().clone()

    res = run_ranks(2, rank_fn, "cpu")
    assert torch.equal(res[0], res[1]) and not ops.qk8_calls and sorted(ops.pv8_calls.values()) == [2, 2]


def test_kv_scale_statement_is_the_two_v_scale_calls():
    from tests import cpu_ops, cpu_ops_sp_qk8

    g = torch.Generator().manual_seed(5)
    y = torch.randn(2, 37, 3 * 2 * 128, generator=g).to(BF)
    k, v = y[:, :, 256:512], y[:, :, 512:]
    v[1, :, :128] = 0
    s = cpu_ops_sp_qk8.kv_scale_fp8(k, v, 2, 128)
    assert s.shape == (2, 2, 2) and torch.equal(s[0], cpu_ops.v_scale_fp8(k, 2, 128)) and torch.equal(s[1], cpu_ops.v_scale_fp8(v, 2, 128))
    assert s[1, 1, 0] == 1.0


def test_kv_scale_fp8_wrapper_checks_before_any_launch(hip_lib, monkeypatch):
    class Refuse:
        def __getattr__(self, name):
            raise RuntimeError("the wrapper reached the library: " + name)

    monkeypatch.setattr(hip_lib, "lib", Refuse())
    B, L, H, hd = 3, 33, 2, 128
    k, v = torch.zeros(B, L, H * hd, dtype=BF), torch.zeros(B, L, H * hd, dtype=BF)
    with pytest.raises(AssertionError):
        hip_lib.kv_scale_fp8(k.float(), v, H, hd)
    with pytest.raises(AssertionError):
        hip_lib.kv_scale_fp8(k, v[:, :-1], H, hd)                                   # k and v of one shape
    with pytest.raises(AssertionError):
        hip_lib.kv_scale_fp8(torch.zeros(B, L, 2 * H * hd, dtype=BF)[:, :, ::2], v, H, hd)      # last dim not contiguous
    with pytest.raises(AssertionError):
        hip_lib.kv_scale_fp8(k, torch.zeros(B, L, H * hd + 4, dtype=BF)[:, :, 4:], H, hd)       # row stride % 8, 16-byte alignment
    with pytest.raises(AssertionError):
        hip_lib.kv_scale_fp8(k, v, H, hd, out=torch.zeros(B, 2, H))                 # [2, B, H], not [B, 2, H]
    with pytest.raises(AssertionError):
        hip_lib.kv_scale_fp8(k, v, H, hd, out=torch.zeros(2, B, H, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="reached the library"):
        hip_lib.kv_scale_fp8(k, v, H, hd)


def test_kv_scale_fp8_entry_refuses_bad_arguments_without_a_launch(hip_lib):
    """status < 0 from the argument checks of the C entry, before any HIP call (no GPU here)"""
    f = hip_lib.lib.osk_kv_scale_fp8
    ok = dict(k=0x1000, kbs=4096, krs=256, v=0x2000, vbs=4096, vrs=256, s=0x3000, B=1, L=16, H=2, hd=128)
    call = lambda **kw: f(*[{**ok, **kw}[n] for n in ("k", "kbs", "krs", "v", "vbs", "vrs", "s", "B", "L", "H", "hd")], None)
    for bad in (dict(k=None), dict(v=None), dict(s=None), dict(k=0x1008), dict(v=0x2004), dict(krs=260), dict(vbs=4100), dict(hd=60),
                dict(H=257), dict(L=0), dict(B=0), dict(s=0x3002)):
        assert call(**bad) < 0, bad
    assert call(hd=8200, krs=16400, vrs=16400) == hip_lib.OSK_EUNSUPPORTED
