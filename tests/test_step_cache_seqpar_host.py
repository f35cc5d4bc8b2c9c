"""CPU: the sampler's step cache under sequence parallelism, host side.  P ranks as threads over tests/local_transport.py on the CPU
statements of the kernels (tests/cpu_ops_step_cache_sp.py): every rank runs I2VDenoiser.denoise(step_cache=...) on its own rows,
the pairs of sums are gathered and combined in rank order, and every rank must take the same decisions from the same floats.
Also: the block stack runs exactly on the steps that are computed, the refusals that remain, a declined split, the sharded
buffers and their key, and the new entry's declaration and binding.  The kernel and the GPU loop: tests/test_gpu_step_cache_seqpar.py."""
import copy
import math
import os
import threading

import pytest
import torch

from oracle import configs, sampling_oracle as S
from tests import cpu_ops_step_cache_sp as SP
from tests.local_transport import LocalTransport, LocalWorld, run_ranks
from tests.test_step_cache_host import SHIPPED, _bf, _model

BF = torch.bfloat16
INF = math.inf
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = 6
_T, _H, _W = 2, 4, 6                          # 2 frames x 2 x 3 = 12 image tokens
L_IMG = _T * (_H // 2) * (_W // 2)


@pytest.fixture()
def sp_ops(hip_lib, monkeypatch):
    from open_sora_amd import mmdit

    for k in ("OSK_STEP_CACHE", "OSK_CFG_PRUNE", "OSK_ATTN_WINDOW_FRAMES", "OSK_SP_KV_CHUNKS", "OSK_SP_MODE"):
        monkeypatch.delenv(k, raising=False)
    mmdit.set_ops_for_testing(SP)
    SP.CALLS.clear()
    SP.SP_CALLS.clear()
    yield mmdit
    mmdit.set_ops_for_testing(hip_lib)


def _case(Lt: int, steps: int = STEPS):
    """the inputs of tests/test_step_cache_host.py::_case with a text length of choice"""
    from open_sora_amd import sampling

    cfg = configs.GOLDEN["hd64_eager_fused"][0]
    n = 1
    g = torch.Generator().manual_seed(11)
    z = torch.randn(n, 16, _T, _H, _W, generator=g).bfloat16().float()
    masks = torch.zeros(n, 1, _T, _H, _W)
    masks[:, :, 0] = 1
    masked_ref = (torch.randn(n, 16, _T, _H, _W, generator=g) * masks).bfloat16().float()
    txt = (torch.randn(3 * n, Lt, cfg["context_in_dim"], generator=g) * 0.2).bfloat16().float()
    y_vec = torch.randn(3 * n, cfg["vec_in_dim"], generator=g).bfloat16().float()
    img_ids, txt_ids = S.grid_ids(3 * n, _T, _H // 2, _W // 2, Lt, torch.float32)
    ts = sampling.get_schedule(steps, (_H // 2) * (_W // 2), _T)
    tensors = dict(img=S.pack(z).repeat(3, 1, 1), masks=masks, masked_ref=masked_ref, img_ids=img_ids, txt=txt, txt_ids=txt_ids, y_vec=y_vec)
    return cfg, tensors, dict(timesteps=ts, **SHIPPED)


def _rank_model(model, world, rank, mode, **enable_kw):
    from open_sora_amd import seqpar

    m = copy.copy(model)                       # shares parameters and plan; own sequence-parallel state, workspaces and step cache
    m.forward = m.forward_ckpt
    object.__setattr__(m, "_osk_ws_cache", {})
    m.__dict__.pop("_osk_step_cache", None)
    tp = LocalTransport(world, rank, "cpu")
    return m, tp, seqpar.enable(m, mode=mode, transport=tp, **enable_kw)


def _run_sp(model, tensors, kw, P, mode, enable_kw=None, **denoise_kw):
    """-> per rank (result, last_step_cache, the rank's model, its transport's call count, its SeqPar, thread ident)"""
    from open_sora_amd import sampling

    def rank_fn(rank, world):
        m, tp, sp = _rank_model(model, world, rank, mode, **(enable_kw or {}))
        den = sampling.I2VDenoiser()
        with torch.inference_mode():
            out = den.denoise(m, **_bf(tensors), **kw, **denoise_kw).float().clone()
        return out, den.last_step_cache, m, tp.calls, sp, threading.get_ident()

    SP.SP_CALLS.clear()                        # (thread idents come back: the record is of this run alone)
    return run_ranks(P, rank_fn, "cpu")


def _split_ok(P: int, L: int, Lt: int) -> bool:
    """the condition under which SeqPar.shard_range keeps the split: rank 0 holds an image row, the last rank a row"""
    Lc = -(-L // P)
    return Lc > Lt and L - (P - 1) * Lc >= 1


# ----------------------------------------------------------------------------- (a) one decision for all ranks
SPLITS = [(2, "allgather", 5), (2, "ulysses", 5), (3, "allgather", 5), (2, "allgather", 4)]   # L = 17 (ragged for 2 and 3) and 16


@pytest.mark.parametrize("P,mode,Lt", SPLITS, ids=[f"P{p}-{m}-Lt{t}" for p, m, t in SPLITS])
def test_every_rank_takes_the_same_decisions_from_the_same_floats(sp_ops, P, mode, Lt):
    cfg, tensors, kw = _case(Lt)
    L = Lt + L_IMG
    assert _split_ok(P, L, Lt) and (Lt == 4 or L % P)
    model = _model(sp_ops, cfg)
    # a threshold inside the range of the accumulated distances: some middle steps skipped, some computed
    probe = _run_sp(model, tensors, kw, P, mode, step_cache=0.0)
    ds = [d for d, _, _ in probe[0][1][1:]]
    assert all(0.0 < d < INF for d in ds)
    res = _run_sp(model, tensors, kw, P, mode, step_cache=1.5 * max(ds))
    rec0 = res[0][1]
    assert len(rec0) == STEPS and rec0[0][0] == INF and rec0[0][2] and rec0[-1][2]
    assert any(not c for _, _, c in rec0) and sum(c for _, _, c in rec0) > 2, rec0
    Lc = -(-L // P)
    for rank, (out, rec, m, calls, sp, ident) in enumerate(res):
        assert rec == rec0, (rank, rec, rec0)                 # tuples of Python floats and bools, compared with ==
        assert torch.equal(out, res[0][0]) and torch.isfinite(out).all()
        assert sp.geom == (Lc, L - (P - 1) * Lc)
        assert SP.SP_CALLS[ident] == [("step_sums_combine", P)] * STEPS
        # sharded buffers: this rank's own image rows, and the rank's row range in the key
        lo, hi = rank * Lc, min((rank + 1) * Lc, L)
        own = (hi - lo) - (min(hi, Lt) - min(lo, Lt))
        sc = m._osk_step_cache
        assert sc.shard == (lo, hi) and sc.key[-3:] == (lo, hi, P)
        assert tuple(sc.prev.shape) == (1, own, cfg["hidden_size"]) and tuple(sc.res.shape) == (3, own, cfg["hidden_size"])
        assert tuple(sc.pairs.shape) == (P, 2) and torch.equal(sc.pairs, res[0][2]._osk_step_cache.pairs)
        assert torch.equal(sc.sums, res[0][2]._osk_step_cache.sums)
    assert sum(r[2]._osk_step_cache.prev.shape[1] for r in res) == L_IMG
    # every step computed: the sharded loop without the cache, bit for bit
    plain = _run_sp(model, tensors, kw, P, mode)
    assert all(torch.equal(p[0], q[0]) for p, q in zip(plain, probe))
    assert not torch.equal(res[0][0], plain[0][0])            # skipping changes the result


def test_with_cfg_prune_and_chunked_gather(sp_ops):
    cfg, tensors, kw = _case(4)
    model = _model(sp_ops, cfg)
    res = _run_sp(model, tensors, kw, 2, "allgather", enable_kw=dict(kv_chunks=2), step_cache=INF, cfg_prune=True)
    assert all(r[1] == res[0][1] and torch.equal(r[0], res[0][0]) for r in res)
    assert [c for _, _, c in res[0][1]] == [i in (0, STEPS - 1) for i in range(STEPS)]


# ----------------------------------------------------------------------------- (b) the block stack runs on the computed steps only
@pytest.mark.parametrize("P", [2, 3])
def test_threshold_inf_runs_the_blocks_on_the_first_and_last_step_only(sp_ops, monkeypatch, P):
    cfg, tensors, kw = _case(5)
    model = _model(sp_ops, cfg)
    per_forward = [r[3] // STEPS for r in _run_sp(model, tensors, kw, P, "allgather")]       # exchanges of one sharded forward
    seen: dict = {}
    real_head, real_blocks = sp_ops.MMDiTModel.step_head, sp_ops.MMDiTModel._forward_blocks

    def head(self, *a, **k):
        seen.setdefault(threading.get_ident(), []).append("head")
        return real_head(self, *a, **k)

    def blocks(self, st):
        seen.setdefault(threading.get_ident(), []).append("blocks")
        assert st.sp is self._sp                              # the blocks get the sp object the head carried
        return real_blocks(self, st)

    monkeypatch.setattr(sp_ops.MMDiTModel, "step_head", head)
    monkeypatch.setattr(sp_ops.MMDiTModel, "_forward_blocks", blocks)
    res = _run_sp(model, tensors, kw, P, "allgather", step_cache=INF)
    want = ["head", "blocks"] + ["head"] * (STEPS - 2) + ["head", "blocks"]
    for out, rec, m, calls, sp, ident in res:
        assert seen[ident] == want
        assert [c for _, _, c in rec] == [i in (0, STEPS - 1) for i in range(STEPS)] and rec == res[0][1]
        assert torch.equal(out, res[0][0])
    # exchanges of a rank: a computed step has the forward's plus the 8-byte gather, a skipped step that gather and the tail's only
    assert all(r[3] == 2 * (f + 1) + (STEPS - 2) * 2 for r, f in zip(res, per_forward)), ([r[3] for r in res], per_forward)


# ----------------------------------------------------------------------------- (c) what stays refused
def test_what_stays_refused(sp_ops):
    from open_sora_amd import sampling, seqpar

    cfg, tensors, kw = _case(4)
    model = _model(sp_ops, cfg)
    tp = lambda: LocalTransport(LocalWorld(2), 0, "cpu")
    run = lambda **extra: sampling.I2VDenoiser().denoise(model, **_bf(tensors), **kw, **extra)
    # hip_graph
    seqpar.enable(model, mode="allgather", transport=tp())
    with pytest.raises(ValueError, match="step_cache and hip_graph=True do not combine"):
        run(step_cache=0.1, hip_graph=True)
    # frame-window attention + sequence parallelism + step cache: through the keyword, a window set on the model, and the model's own entry
    triple = "step_cache: frame-window attention, sequence parallelism and the step cache do not run together"
    with pytest.raises(ValueError, match=triple):
        run(step_cache=0.1, attn_window_frames=1)
    assert model._attn_window is None                          # refused before the window was set
    model.set_attention_window(1, 6)
    with pytest.raises(ValueError, match=triple):
        run(step_cache=0.1)
    with pytest.raises(ValueError, match=triple):
        model.step_cache_begin(1, 3, L_IMG, "cpu", L_txt=4)
    model.set_attention_window(None)
    sc = model.step_cache_begin(1, 3, L_IMG, "cpu", L_txt=4)      # without the window: accepted
    model.set_attention_window(1, 6)
    with pytest.raises(ValueError, match=triple):
        model.step_head(sc, **{k: v for k, v in _bf(tensors).items() if k not in ("masks", "masked_ref")}, timesteps=torch.zeros(3, dtype=BF))
    model.set_attention_window(None)
    with pytest.raises(ValueError, match="L_txt"):
        model.step_cache_begin(1, 3, L_IMG, "cpu")
    # an sp object that does not declare the capability: the messages from before, word for word
    model._sp = object()
    with pytest.raises(ValueError) as e:
        run(step_cache=0.1)
    assert str(e.value) == "step_cache does not run under sequence parallelism (every rank would have to take the same decision)"
    with pytest.raises(ValueError) as e:
        model.step_cache_begin(1, 3, L_IMG, "cpu")
    assert str(e.value) == ("step_cache: a model under sequence parallelism is out of scope for the step cache (every rank would "
                            "need the same distance); run it without seqpar.enable or leave step_cache off")
    with pytest.raises(ValueError) as e:
        model.step_head(sc, None, None, None, None, None, None)
    assert str(e.value) == "step_cache: a model under sequence parallelism is out of scope for the step cache"
    assert seqpar.SeqPar.step_cache is True and seqpar.SeqPar.kv_qk8 is True
    assert not SP.SP_CALLS and not SP.CALLS


# ----------------------------------------------------------------------------- (d) a declined split
def test_a_declined_split_runs_the_single_device_step(sp_ops):
    """12 text + 12 image rows over P = 2: ceil(24 / 2) = 12 rows would leave rank 0 without an image row, shard_range declines, and
    every rank runs the whole step on the existing path -- no exchange at all, the single-device cache, the single-device bits"""
    from open_sora_amd import sampling

    Lt = 12
    cfg, tensors, kw = _case(Lt)
    assert not _split_ok(2, Lt + L_IMG, Lt)
    model = _model(sp_ops, cfg)
    with torch.inference_mode():
        den = sampling.I2VDenoiser()
        single = den.denoise(model, step_cache=INF, **_bf(tensors), **kw).float().clone()
    model.__dict__.pop("_osk_step_cache", None)
    res = _run_sp(model, tensors, kw, 2, "allgather", step_cache=INF)
    for out, rec, m, calls, sp, ident in res:
        assert calls == 0 and sp.geom is None and ident not in SP.SP_CALLS
        sc = m._osk_step_cache
        assert sc.shard is None and sc.pairs is None and tuple(sc.prev.shape) == (1, L_IMG, cfg["hidden_size"]) and len(sc.key) == 7
        assert rec == den.last_step_cache and torch.equal(out, single)


# ----------------------------------------------------------------------------- the combine: statement and binding
def test_combine_statement_adds_in_rank_order():
    pairs = torch.tensor([[1.0, 2.0 ** 24], [2.0 ** -24, 1.0], [1.0, 1.0]])
    sums = torch.zeros(2)
    SP.step_sums_combine(pairs, sums)
    # (1 + 2^-24) rounds to 1, then + 1 = 2;  (2^24 + 1) rounds to 2^24 (ties to even), then + 1 again: the order is visible
    assert sums.tolist() == [2.0, 2.0 ** 24]
    assert SP.step_sums_combine_f64(pairs) == (2.0 + 2.0 ** -24, 2.0 ** 24 + 2.0)
    SP.step_sums_combine(torch.tensor([[3.0, float("nan")], [float("inf"), 1.0]]), sums)
    assert sums[0] == INF and math.isnan(float(sums[1]))
    with pytest.raises(RuntimeError, match="osk_step_sums_combine_f32"):
        SP.step_sums_combine(pairs, pairs[1])                  # overlap
    with pytest.raises(RuntimeError, match="osk_step_sums_combine_f32"):
        SP.step_sums_combine(pairs.double(), sums)


def test_entry_point_is_declared_bound_and_validates_before_any_launch(hip_lib):
    with open(os.path.join(ROOT, "include", "osk.h")) as f:
        header = f.read()
    assert "int osk_step_sums_combine_f32(const float* pairs, int P, float* sums, void* stream);" in header
    assert "#define OSK_ABI_VERSION 2" in header and hip_lib.lib.osk_abi_version() == 2
    assert len(hip_lib.SIGNATURES["osk_step_sums_combine_f32"]) == 4 and callable(hip_lib.step_sums_combine)
    with pytest.raises(ValueError, match="osk_step_sums_combine_f32"):
        hip_lib.step_sums_combine(torch.zeros(2, 2), torch.zeros(2))        # CPU tensors
    lib = hip_lib.lib
    assert lib.osk_step_sums_combine_f32(None, 2, 0x2000, None) < 0
    assert lib.osk_step_sums_combine_f32(0x1000, 2, None, None) < 0
    assert lib.osk_step_sums_combine_f32(0x1000, 0, 0x2000, None) < 0           # P < 1
    assert lib.osk_step_sums_combine_f32(0x1002, 2, 0x2000, None) < 0           # alignment
    assert lib.osk_step_sums_combine_f32(0x1000, 2, 0x2001, None) < 0
