"""CPU: attention broadcast under sequence parallelism, host side.  P ranks as threads over tests/local_transport.py on the CPU
statements of the kernels (tests/cpu_ops_attn_broadcast.py): every rank keeps the attention outputs of its own rows, a reuse step
exchanges nothing inside the blocks -- the one collective left is the tail's gather of the prediction -- and the gathered
prediction is the single-device reuse step's within the bound the suite holds a sharded forward to (tests/test_seqpar_window_host.py:
2^-7 relative L2).  The GPU pair: tests/test_gpu_attn_broadcast_seqpar.py."""
import copy

import pytest
import torch

from oracle import configs
from tests import cpu_ops_attn_broadcast as AB
from tests.local_transport import LocalTransport, run_ranks
from tests.util import rel_l2, torch_inputs, torch_params

BF = torch.bfloat16
B_, T_, H_, W_ = 2, 2, 4, 6                      # 2 frames x 24 = 48 image tokens
L_IMG = T_ * H_ * W_
SHARDED_BOUND = 2.0 ** -7                        # tests/test_seqpar_window_host.py / tests/test_seqpar_chunked_host.py


@pytest.fixture()
def ab_ops(hip_lib, monkeypatch):
    from open_sora_amd import mmdit

    for k in ("OSK_ATTN_BROADCAST", "OSK_STEP_CACHE", "OSK_CFG_PRUNE", "OSK_ATTN_WINDOW_FRAMES", "OSK_SP_KV_CHUNKS", "OSK_SP_MODE"):
        monkeypatch.delenv(k, raising=False)
    mmdit.set_ops_for_testing(AB)
    AB.AB_CALLS.clear()
    yield mmdit
    mmdit.set_ops_for_testing(hip_lib)


def _model(mmdit, heads=None):
    cfg = dict(configs.GOLDEN["hd72_eager_split"][0], depth=2, depth_single_blocks=2)
    if heads is not None:
        cfg = dict(configs.GOLDEN["hd64_eager_fused"][0], depth=2, depth_single_blocks=2, hidden_size=64 * heads, num_heads=heads)
    model = mmdit.Flux(device_map="cpu", torch_dtype=BF, **cfg)
    model.load_state_dict(torch_params(cfg, dtype=BF), strict=True)
    return cfg, model


def _shift(inp, s):
    return dict(inp, img=(inp["img"].float() * (1.0 + s)).to(BF), timesteps=(inp["timesteps"].float() * (1.0 - s)).to(BF))


def _pair(model, a, b, Lt, rows):
    """store on a, reuse on b -> (store's prediction, reuse's, the cache)"""
    ac = model.attention_broadcast_begin(len(rows), Lt, L_IMG, "cpu")
    s = model(**a, attn_cache=(ac, "store", rows)).float().clone()
    r = model(**b, attn_cache=(ac, "reuse", rows)).float().clone()
    return s, r, ac


def _run_sp(model, a, b, Lt, P, mode, rows):
    """-> per rank (store's prediction, reuse's, collectives of the plain / store / reuse forward, the cache, the SeqPar)"""
    from open_sora_amd import seqpar

    def rank_fn(rank, world):
        m = copy.copy(model)                       # shares parameters and plan; own sequence-parallel state, workspaces and cache
        m.forward = m.forward_ckpt
        object.__setattr__(m, "_osk_ws_cache", {})
        m.__dict__.pop("_osk_attn_cache", None)
        tp = LocalTransport(world, rank, "cpu")
        sp = seqpar.enable(m, mode=mode, transport=tp)
        with torch.inference_mode():
            m(**a)
            n_plain = tp.calls
            ac = m.attention_broadcast_begin(len(rows), Lt, L_IMG, "cpu")
            s = m(**a, attn_cache=(ac, "store", rows)).float().clone()
            n_store = tp.calls - n_plain
            r = m(**b, attn_cache=(ac, "reuse", rows)).float().clone()
            n_reuse = tp.calls - n_plain - n_store
        return s, r, (n_plain, n_store, n_reuse), ac, sp

    return run_ranks(P, rank_fn, "cpu")


# (P, mode, text length, heads or None = the 8 heads of the hd 72 model): L = Lt + 48.  Even: 56 / 2, 56 / 4; ragged: 53 over 2 (27, 26),
# 57 over 4 (15, 15, 15, 12).  Head exchange at P = 4 needs a head count 4 divides: 8 does.
SPLITS = [(2, "allgather", 8, None), (2, "ulysses", 8, None), (2, "allgather", 5, None), (2, "ulysses", 5, None),
          (4, "allgather", 8, None), (4, "ulysses", 8, None), (4, "allgather", 9, None), (4, "ulysses", 9, None)]


@pytest.mark.parametrize("P,mode,Lt,heads", SPLITS, ids=[f"P{p}-{m}-L{t + L_IMG}" for p, m, t, _ in SPLITS])
def test_reuse_step_exchanges_nothing_inside_the_blocks(ab_ops, P, mode, Lt, heads):
    cfg, model = _model(ab_ops, heads)
    a = torch_inputs(cfg, B_, T_, H_, W_, Lt, dtype=BF)
    b = _shift(a, 0.125)
    rows = (0, 1)
    L = Lt + L_IMG
    Lc = -(-L // P)
    assert Lc > Lt and L - (P - 1) * Lc >= 1, "the split must be kept"
    with torch.inference_mode():
        plain_b = model(**b).float().clone()
        single_store, single_reuse, ac1 = _pair(model, a, b, Lt, rows)
    assert tuple(ac1.slots.shape) == (4, B_, L, cfg["hidden_size"]) and ac1.shard is None
    res = _run_sp(model, a, b, Lt, P, mode, rows)
    for rank, (s, r, (n_plain, n_store, n_reuse), ac, sp) in enumerate(res):
        assert sp.geom == (Lc, L - (P - 1) * Lc)
        assert torch.equal(s, res[0][0]) and torch.equal(r, res[0][1])
        # a plain and a store forward exchange inside every block; a reuse forward only gathers the prediction
        assert n_store == n_plain > 1 + 4 and n_reuse == 1, (n_plain, n_store, n_reuse)
        lo, hi = rank * Lc, min((rank + 1) * Lc, L)
        assert ac.shard == (lo, hi) and ac.key[-3:] == (lo, hi, P) and tuple(ac.slots.shape) == (4, B_, hi - lo, cfg["hidden_size"])
        assert ac.have == [True, True]
    assert sum(r[3].slots.shape[2] for r in res) == L
    e_store, e_reuse = rel_l2(res[0][0], single_store), rel_l2(res[0][1], single_reuse)
    sep = rel_l2(single_reuse, plain_b)
    print(f"P = {P} {mode} L = {L}: relL2 sharded vs single-device store {e_store:.3e}, reuse {e_reuse:.3e}; reuse vs its plain step {sep:.3e}")
    assert e_store <= SHARDED_BOUND and e_reuse <= SHARDED_BOUND
    assert sep > 0.0


def test_sampler_loop_takes_the_same_modes_on_every_rank(ab_ops):
    """the schedule is a pure function of the step index: every rank runs the same modes with nothing to agree on, and the sharded
    loop's result is the single-device loop's within the sharded bound"""
    from open_sora_amd import sampling, seqpar
    from tests.test_step_cache_host import _bf, _model as _sc_model
    from tests.test_step_cache_seqpar_host import _case

    cfg, tensors, kw = _case(4, 6)
    model = _sc_model(ab_ops, cfg)
    opts = dict(attn_broadcast=2, attn_broadcast_range=(0.0, 1.0))
    with torch.inference_mode():
        den = sampling.I2VDenoiser()
        single = den.denoise(model, **opts, **_bf(tensors), **kw).float().clone()
    want = den.last_attn_broadcast
    assert want == ["plain", "store", "reuse", "store", "reuse", "plain"]

    def rank_fn(rank, world):
        m = copy.copy(model)
        m.forward = m.forward_ckpt
        object.__setattr__(m, "_osk_ws_cache", {})
        m.__dict__.pop("_osk_attn_cache", None)
        tp = LocalTransport(world, rank, "cpu")
        seqpar.enable(m, mode="allgather", transport=tp)
        d = sampling.I2VDenoiser()
        with torch.inference_mode():
            out = d.denoise(m, **opts, **_bf(tensors), **kw).float().clone()
        return out, d.last_attn_broadcast, tp.calls

    res = run_ranks(2, rank_fn, "cpu")
    assert all(r[1] == want and torch.equal(r[0], res[0][0]) for r in res)
    per_block_forward = (res[0][2] - 6) // 4               # 4 forwards exchange inside their blocks, all 6 gather the prediction
    assert res[0][2] == 6 + 4 * per_block_forward and per_block_forward >= 5
    e = rel_l2(res[0][0], single)
    print(f"sharded attention-broadcast loop vs single device: relL2 {e:.3e}")
    assert e <= SHARDED_BOUND
