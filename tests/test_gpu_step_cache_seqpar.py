"""GPU: the sampler's step cache under sequence parallelism, P ranks as threads of this process on the one GPU
(tests/local_transport.py).  (1) osk_step_sums_combine_f32 (csrc/step_cache.hip) against f64 within the P roundings of its P - 1
adds, NaN propagation, guard bands, bit-equal repeats, refused arguments; (2) the combined sums of a sharded step_head against the
f64 distance of the ranks' own rows put together, bit-equal on every rank; (3) step_cache=0.0 under sequence parallelism is the
sharded loop without the cache bit for bit; (4) step_cache=inf meets the parity rule of tests/util.py against the same fp32
statement and CPU comparator as the single-device test (tests/test_gpu_step_cache.py), every rank returning the same bits and the
same decisions; (5) a pruned loop computes where a row has no residual, the same on all ranks.  Every split keeps ceil(L / P) above
the text length, so none is declined (the declined split: tests/test_step_cache_seqpar_host.py).  Each check prints its measured
figure before it asserts (pytest -s)."""
import copy
import functools
import math

import pytest
import torch

from oracle import configs
from tests import cpu_ops_step_cache_sp as SP
from tests.local_transport import LocalTransport, run_ranks
from tests.test_gpu_mmdit import _build
from tests.test_gpu_row_kernels import assert_guards, bits, guarded
from tests.test_gpu_step_cache import MIDDLE_SKIPPED, STEPS, _case, _references, _to, chain
from tests.util import assert_parity, torch_params

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF = torch.bfloat16
INF = math.inf
L_TXT, L_IMG = 32, 72                       # tests/test_gpu_step_cache.py::_case: 3 frames x 6 x 4 image tokens behind 32 text tokens
# head exchange needs a head count P divides: 8 heads take P = 2; P = 3 runs on a three-head model of the same inputs
CFG3 = ("hd128_liger_split", (("hidden_size", 384), ("num_heads", 3)))


def _split(P: int, L: int = L_TXT + L_IMG):
    """(Lc, Ltail) of SeqPar.split, with the condition under which shard_range keeps the split"""
    Lc = -(-L // P)
    assert Lc > L_TXT and L - (P - 1) * Lc >= 1, "the split would be declined"
    return Lc, L - (P - 1) * Lc


def _own_image_rows(P: int, rank: int) -> int:
    Lc, _ = _split(P)
    lo, hi = rank * Lc, min((rank + 1) * Lc, L_TXT + L_IMG)
    return (hi - lo) - (min(hi, L_TXT) - min(lo, L_TXT))


# ----------------------------------------------------------------------------- (1) the combine kernel
def _pairs(kind: str, P: int) -> torch.Tensor:
    g = torch.Generator().manual_seed(97 * P + len(kind))
    p = torch.randn(P, 2, generator=g).abs() * 1e4 + 1.0           # sums of absolute values: positive
    if kind == "magnitudes":
        p = torch.where(torch.arange(2 * P).view(P, 2) % 3 == 0, torch.full((P, 2), 1e6), torch.full((P, 2), 1e-3)) * (1 + p / 1e6)
    if kind == "nan":
        p[P // 2, 1] = float("nan")
    return p.float()


@pytest.mark.parametrize("kind", ["random", "magnitudes", "nan"])
@pytest.mark.parametrize("P", [1, 2, 3, 8])
def test_sums_combine_vs_f64(hip_lib, P, kind):
    pairs0 = _pairs(kind, P)
    flat_p, pairs = guarded(2 * P, torch.float32)
    pairs = pairs.view(P, 2)
    pairs.copy_(pairs0)
    flat_s, sums = guarded(2, torch.float32)
    hip_lib.step_sums_combine(pairs, sums)
    torch.cuda.synchronize()
    assert_guards(flat_p, 2 * P)
    assert_guards(flat_s, 2)
    assert torch.equal(bits(pairs.cpu()), bits(pairs0)), "pairs was written"
    got = [float(v) for v in sums.double().cpu()]
    want = SP.step_sums_combine_f64(pairs0)
    for j in range(2):
        if math.isnan(want[j]):
            assert math.isnan(got[j]), (kind, P, got)
            continue
        # P - 1 adds of positive terms: each rounds by at most 2^-24 of a partial sum, which is at most the total
        e = abs(got[j] - want[j]) / want[j]
        print(f"sums_combine {kind} P = {P} column {j}: rel err {e:.3e}; allowed P x 2^-24 = {P * 2.0 ** -24:.3e}")
        assert e <= P * 2.0 ** -24
    # the CPU statement adds in the same order: the same bits (a NaN's payload aside)
    cpu = torch.zeros(2)
    SP.step_sums_combine(pairs0, cpu)
    assert torch.equal(bits(sums.cpu().nan_to_num(nan=-1.0)), bits(cpu.nan_to_num(nan=-1.0)))
    sums2 = torch.zeros(2, device=DEV)
    hip_lib.step_sums_combine(pairs, sums2)
    torch.cuda.synchronize()
    assert torch.equal(bits(sums.cpu()), bits(sums2.cpu()))


def test_sums_combine_refused_arguments_launch_nothing(hip_lib):
    flat_p, pairs = guarded(6, torch.float32)
    pairs = pairs.view(3, 2)
    flat_s, sums = guarded(2, torch.float32)
    before_p, before_s = flat_p.clone(), flat_s.clone()
    wide = torch.zeros(3, 4, device=DEV)
    for bad in (lambda: hip_lib.step_sums_combine(pairs.double(), sums),
                lambda: hip_lib.step_sums_combine(wide[:, :2], sums),                    # not contiguous
                lambda: hip_lib.step_sums_combine(pairs[:0], sums),                      # P = 0
                lambda: hip_lib.step_sums_combine(pairs.view(-1), sums),                 # not [P, 2]
                lambda: hip_lib.step_sums_combine(pairs, pairs[1]),                      # overlap
                lambda: hip_lib.step_sums_combine(pairs, torch.zeros(3, device=DEV)),
                lambda: hip_lib.step_sums_combine(pairs.cpu(), sums)):
        with pytest.raises(ValueError, match="osk_step_sums_combine_f32"):
            bad()
    lib = hip_lib.lib
    assert lib.osk_step_sums_combine_f32(pairs.data_ptr(), 0, sums.data_ptr(), None) < 0
    assert lib.osk_step_sums_combine_f32(None, 3, sums.data_ptr(), None) < 0
    assert lib.osk_step_sums_combine_f32(pairs.data_ptr(), 3, None, None) < 0
    assert lib.osk_step_sums_combine_f32(pairs.data_ptr() + 2, 3, sums.data_ptr(), None) < 0
    assert lib.osk_step_sums_combine_f32(pairs.data_ptr(), 3, sums.data_ptr() + 1, None) < 0
    torch.cuda.synchronize()
    assert torch.equal(bits(flat_p), bits(before_p)) and torch.equal(bits(flat_s), bits(before_s))


# ----------------------------------------------------------------------------- ranks as threads
@functools.lru_cache(maxsize=None)
def _model(which=None):
    """the small denoiser on the GPU, its plan built (shared and read-only once the rank threads start)"""
    cfg, tensors, kw = _case()
    if which is not None:
        cfg = dict(configs.GOLDEN[which[0]][0], **dict(which[1]))
    model = _build(cfg, DEV)
    with torch.inference_mode():
        model(**_head_inputs(tensors, kw["timesteps"][0], 0.0))
    torch.cuda.synchronize()
    return cfg, model


def _head_inputs(tensors, t: float, shift: float) -> dict:
    """the keyword arguments the sampler hands the model for the CFG triple (sampling.I2VDenoiser.denoise), latents moved by `shift`"""
    from open_sora_amd import sampling

    d = _to(tensors, DEV)
    cond = sampling.pack(torch.cat((d["masks"], d["masked_ref"]), dim=1))
    n3 = d["img"].shape[0]
    return dict(img=(d["img"].float() * (1.0 + shift)).to(BF), img_ids=d["img_ids"], txt=d["txt"], txt_ids=d["txt_ids"], y_vec=d["y_vec"],
                cond=torch.cat([cond, cond, torch.zeros_like(cond)], 0), timesteps=torch.full((n3,), t, device=DEV, dtype=BF),
                guidance=torch.full((n3,), 7.5, device=DEV, dtype=BF))


def _rank_model(model, world, rank, mode):
    from open_sora_amd import seqpar

    m = copy.copy(model)                       # shares parameters and plan; own sequence-parallel state, workspaces and step cache
    m.forward = m.forward_ckpt
    object.__setattr__(m, "_osk_ws_cache", {})
    m.__dict__.pop("_osk_step_cache", None)
    sp = seqpar.enable(m, mode=mode, transport=LocalTransport(world, rank, DEV))
    assert m._sp is sp and sp.rank == rank
    return m, sp


def _run_sp(model, tensors, kw, P, mode, **denoise_kw):
    """-> per rank (result on the CPU, last_step_cache, the rank's model)"""
    from open_sora_amd import sampling

    def rank_fn(rank, world):
        m, sp = _rank_model(model, world, rank, mode)
        den = sampling.I2VDenoiser()
        with torch.inference_mode():
            out = den.denoise(m, **_to(tensors, DEV), **kw, **denoise_kw)
        torch.cuda.current_stream().synchronize()
        assert sp.geom == _split(P)
        return out.cpu(), den.last_step_cache, m

    return run_ranks(P, rank_fn, DEV)


def _assert_ranks_agree(res):
    for out, rec, _ in res[1:]:
        assert torch.equal(bits(out), bits(res[0][0])), "ranks disagree on the result"
        assert rec == res[0][1], "ranks disagree on (d, acc, computed)"          # Python floats, compared with ==


# ----------------------------------------------------------------------------- (2) the sharded distance is the distance
@pytest.mark.parametrize("P", [2, 3])
def test_sharded_distance_is_the_distance(hip_lib, P):
    cfg, tensors, kw = _case()
    _, model = _model()
    assert P == 2 or _split(P)[0] != _split(P)[1]                    # P = 3: a ragged split
    ts = kw["timesteps"]

    def rank_fn(rank, world):
        m, sp = _rank_model(model, world, rank, "allgather")
        with torch.inference_mode():
            sc = m.step_cache_begin(1, 3, L_IMG, DEV, L_txt=L_TXT)
            m.step_head(sc, **_head_inputs(tensors, ts[0], 0.0))
            before = sc.prev.clone()
            st = m.step_head(sc, **_head_inputs(tensors, ts[1], 0.05))
            cur = st.ws.xm[:1, st.ws.L_txt:].clone()
            d = m.step_distance(sc)
        torch.cuda.current_stream().synchronize()
        assert tuple(sc.prev.shape) == (1, _own_image_rows(P, rank), cfg["hidden_size"]) and tuple(sc.pairs.shape) == (P, 2)
        assert torch.equal(bits(sc.prev), bits(cur)), "prev is not this rank's M_i afterwards"
        return cur.cpu(), before.cpu(), sc.sums.cpu(), sc.pairs.cpu(), d

    res = run_ranks(P, rank_fn, DEV)
    cur = torch.cat([r[0] for r in res], 1)
    before = torch.cat([r[1] for r in res], 1)
    assert cur.shape[1] == L_IMG and float(before.float().abs().sum()) > 0.0
    num64, den64 = SP.step_delta_f64(cur, before)
    k = chain(1, max(_own_image_rows(P, r) for r in range(P)), cfg["hidden_size"]) + P
    num, den = (float(v) for v in res[0][2].double())
    e_num, e_den = abs(num - num64) / num64, abs(den - den64) / den64
    print(f"sharded distance P = {P}: rel err num {e_num:.3e} den {e_den:.3e}; allowed {k} x 2^-24 = {k * 2.0 ** -24:.3e}; d = {res[0][4]:.5f}")
    assert e_num <= k * 2.0 ** -24 and e_den <= k * 2.0 ** -24
    for r in res[1:]:
        assert torch.equal(bits(r[2]), bits(res[0][2])) and torch.equal(bits(r[3]), bits(res[0][3])) and r[4] == res[0][4]
    # slot r of the gathered pairs is rank r's own share
    for rank, r in enumerate(res):
        own = SP.step_delta_f64(r[0], r[1])
        kr = chain(1, _own_image_rows(P, rank), cfg["hidden_size"])
        assert all(abs(float(r[3][rank, j]) - own[j]) <= kr * 2.0 ** -24 * own[j] for j in range(2))


# ----------------------------------------------------------------------------- (3) threshold 0 is the sharded loop without the cache
@pytest.mark.parametrize("mode", ["allgather", "ulysses"])
def test_threshold_zero_is_the_sharded_loop_bit_for_bit(hip_lib, monkeypatch, mode):
    monkeypatch.delenv("OSK_STEP_CACHE", raising=False)
    cfg, tensors, kw = _case()
    _, model = _model()
    plain = _run_sp(model, tensors, kw, 2, mode)
    cached = _run_sp(model, tensors, kw, 2, mode, step_cache=0.0)
    _assert_ranks_agree(plain)
    _assert_ranks_agree(cached)
    assert plain[0][1] is None and torch.isfinite(plain[0][0].float()).all()
    assert torch.equal(bits(plain[0][0]), bits(cached[0][0]))
    rec = cached[0][1]
    print("distances:", " ".join(f"{d:.4f}" for d, _, _ in rec))
    assert len(rec) == STEPS and all(c for _, _, c in rec) and rec[0][0] == INF and all(0.0 < d < INF for d, _, _ in rec[1:])


# ----------------------------------------------------------------------------- (4) threshold inf meets the parity rule
@functools.lru_cache(maxsize=None)
def _references3():
    """tests/test_gpu_step_cache.py::_references(False) for the three-head model: the fp32 statement of the step-cached loop at
    threshold +inf and the CPU kernel table's single-device bf16 run of the same loop; computed once, left unchanged"""
    from open_sora_amd import mmdit, sampling

    _, tensors, kw = _case()
    cfg = dict(configs.GOLDEN[CFG3[0]][0], **dict(CFG3[1]))
    with torch.inference_mode():
        a = dict(tensors)
        truth, record = SP.i2v_denoise_step_cache(torch_params(cfg), cfg, a.pop("img"), counts=[3] * STEPS, threshold=INF, **a, **kw)
        hip = mmdit.ops()
        mmdit.set_ops_for_testing(SP)
        try:
            model = mmdit.Flux(device_map="cpu", torch_dtype=BF, **cfg)
            model.load_state_dict(torch_params(cfg, dtype=BF), strict=True)
            emu = sampling.I2VDenoiser().denoise(model, step_cache=INF, **_to(tensors, "cpu"), **kw)
        finally:
            mmdit.set_ops_for_testing(hip)
    return truth, record, emu, [3] * STEPS


INF_CASES = [(2, "allgather", False, None), (2, "ulysses", False, None), (3, "allgather", False, None), (3, "ulysses", False, CFG3),
             (3, "allgather", True, None)]


@pytest.mark.parametrize("P,mode,pruned,which", INF_CASES,
                         ids=[f"P{p}-{m}{'-cfg_prune' if pr else ''}{'-3heads' if w else ''}" for p, m, pr, w in INF_CASES])
def test_threshold_inf_skips_the_middle_steps_and_meets_parity(hip_lib, P, mode, pruned, which):
    """the reference of tests/test_gpu_step_cache.py's test of the same name: the oracle's fp32 loop with the same skip pattern, judged
    against the single-device CPU comparator -- neither comes from the sharded code.  8 heads do not divide by 3 (SeqPar.head_parallel
    asserts it), so head exchange at P = 3 runs a three-head model on the same inputs, with references made the same way."""
    cfg, tensors, kw = _case()
    truth, record, emu, counts = _references(pruned) if which is None else _references3()
    cfg, model = _model(which)
    assert cfg["num_heads"] % P == 0 or mode == "allgather"
    res = _run_sp(model, tensors, kw, P, mode, step_cache=INF, cfg_prune=pruned)
    _assert_ranks_agree(res)
    rec = res[0][1]
    assert [c for _, _, c in rec] == MIDDLE_SKIPPED == [c for _, _, c in record]
    assert not pruned or sorted(set(counts)) == [1, 3]
    for rank, (_, _, m) in enumerate(res):
        assert m._sp.head_parallel(cfg["num_heads"]) == (mode == "ulysses")
        assert m._osk_step_cache.prev.shape[1] == _own_image_rows(P, rank)
    assert_parity(res[0][0], truth, emu, f"step-cached loop under sequence parallelism, P = {P} {mode}{' pruned' if pruned else ''}, {STEPS} steps, "
                                         f"2 computed, vs the fp32 statement; comparator: the CPU kernel table on one device")


# ----------------------------------------------------------------------------- (5) residuals per row under cfg_prune
def test_pruned_loop_computes_where_a_row_has_no_residual(hip_lib, monkeypatch):
    """tests/test_gpu_step_cache.py's test of the same name on two ranks: branch counts that START on one branch -- step 0 and step 2
    (rows 1 and 2 hold nothing yet) are computed, everything up to the last step is skipped, on both ranks alike"""
    from open_sora_amd import sampling

    counts = [1, 1, 3, 1, 3, 3, 1, 3, 1, 1, 3, 1, 3, 1]
    monkeypatch.setattr(sampling, "cfg_branch_counts", lambda *a, **k: list(counts))
    cfg, tensors, kw = _case()
    _, model = _model()
    res = _run_sp(model, tensors, kw, 2, "allgather", step_cache=INF, cfg_prune=True)
    _assert_ranks_agree(res)
    for out, rec, m in res:
        assert [c for _, _, c in rec] == [i in (0, 2, STEPS - 1) for i in range(STEPS)]
        assert torch.isfinite(out.float()).all() and m._osk_step_cache.have == [True] * 3
