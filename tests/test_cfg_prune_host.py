"""CPU: the host side of CFG branch pruning (I2VDenoiser.denoise(cfg_prune=True), open_sora_amd/sampling.py): the branch plan,
the loop around a stub model that records the batch it is called with, duplicate-branch detection from the tensors, the
untouched default path, the environment switch, sequence-parallel ranks as threads, and the binding of osk_cfg_euler_nb_bf16.
Kernels are emulated by tests/cpu_ops_cfg_prune.py; the kernel itself is checked on the GPU by tests/test_gpu_cfg_prune.py."""
import copy
import os

import pytest
import torch

from oracle import configs, sampling_oracle as S
from tests import cpu_ops_cfg_prune as P
from tests.local_transport import LocalTransport, run_ranks
from tests.util import assert_parity, torch_params

BF = torch.bfloat16
F64 = torch.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIPPED = dict(guidance=7.5, guidance_img=3.0, text_osci=True, image_osci=True, scale_temporal_osci=True)   # 256px.py:20-28
ODD_FROM_11 = lambda steps: [i for i in range(steps) if i >= 11 and i % 2]


@pytest.fixture()
def prune_ops(hip_lib, monkeypatch):
    from open_sora_amd import mmdit

    monkeypatch.delenv("OSK_CFG_PRUNE", raising=False)
    mmdit.set_ops_for_testing(P)
    P.CALLS.clear()
    yield mmdit
    mmdit.set_ops_for_testing(hip_lib)


# ----------------------------------------------------------------------------- the plan
def test_branch_plan_on_the_shipped_settings():
    from open_sora_amd.sampling import cfg_branch_counts

    ones = ODD_FROM_11(50)
    assert len(ones) == 20 and ones[0] == 11 and ones[-1] == 49
    c = cfg_branch_counts(50, dup23=False, **SHIPPED)
    assert c == [1 if i in ones else 3 for i in range(50)] and c.count(3) == 30 and c.count(1) == 20
    c = cfg_branch_counts(50, dup23=True, **SHIPPED)
    assert c == [1 if i in ones else 2 for i in range(50)] and c.count(2) == 30 and c.count(1) == 20
    for dup in (False, True):
        assert cfg_branch_counts(50, **dict(SHIPPED, guidance=1.0, guidance_img=1.0), dup23=dup) == [1] * 50
    assert cfg_branch_counts(50, 7.5, 1.0, False, False, False, False) == [2] * 50
    assert cfg_branch_counts(50, 7.5, 1.0, False, False, True, False) == [2] * 50     # (no ramp at image_gs == 1.0)
    # text guidance 1.0 but the temporal ramp active: u2 does not cancel
    assert cfg_branch_counts(6, 1.0, 3.0, False, False, True, False) == [3] * 6
    assert cfg_branch_counts(6, 1.0, 3.0, False, False, True, True) == [1] * 6
    assert cfg_branch_counts(6, 1.0, 3.0, False, False, False, False) == [3] * 6


# ----------------------------------------------------------------------------- the loop around a stub model
N, STEPS = 2, 14
_T, _H, _W, _LT = 2, 4, 6, 5
_W_STUB = torch.randn(64 + 68, 64, generator=torch.Generator().manual_seed(5), dtype=F64) * 0.02


def _stub(batches):
    """the stub of tests/test_host_orchestration.py::test_sampler_loop_matches_reference_formula: row-independent, records the
    batch of every call, and insists that every tripled keyword arrives cut to that batch"""
    def model(img, cond, timesteps, guidance, **kw):
        B = img.shape[0]
        batches.append(B)
        assert cond.shape[0] == B and timesteps.shape[0] == B and guidance.shape[0] == B
        assert all(v.shape[0] == B for v in kw.values() if torch.is_tensor(v)), {k: tuple(v.shape) for k, v in kw.items()}
        dt = img.dtype
        return (torch.cat([img.to(F64), cond.to(F64)], -1) @ _W_STUB * (1 + timesteps.to(F64)[:, None, None])).to(dt)
    return model


def _inputs(t2v=False, seed=0):
    from open_sora_amd import sampling

    g = torch.Generator().manual_seed(seed)
    z = torch.randn(N, 16, _T, _H, _W, generator=g).to(BF)
    masks = torch.zeros(N, 1, _T, _H, _W, dtype=BF)
    if not t2v:
        masks[:, :, 0] = 1
    masked_ref = (torch.randn(N, 16, _T, _H, _W, generator=g) * masks.float()).to(BF)
    txt = torch.randn(3 * N, _LT, 8, generator=g).to(BF)
    y_vec = torch.randn(3 * N, 6, generator=g).to(BF)
    if t2v:                                                  # prepare_guidance: text + neg + neg
        txt[2 * N:] = txt[N:2 * N]
        y_vec[2 * N:] = y_vec[N:2 * N]
    img_ids, txt_ids = sampling.prepare_ids(3 * N, _T, _H, _W, _LT, "cpu", BF)
    ts = sampling.get_schedule(STEPS, (_H // 2) * (_W // 2), _T)
    return dict(img=sampling.pack(z).repeat(3, 1, 1), masks=masks, masked_ref=masked_ref, txt=txt, txt_ids=txt_ids, y_vec=y_vec,
                img_ids=img_ids, timesteps=ts, sigma_min=1e-5, **SHIPPED)


def _run(args, **extra):
    from open_sora_amd import sampling

    batches = []
    den = sampling.I2VDenoiser()
    out = den.denoise(_stub(batches), **dict(args), **extra)
    return out, batches, den


def _f64_loop(args):
    """opensora/utils/sampling.py:181-222 in f64 around the same stub: no rounding anywhere"""
    from open_sora_amd import sampling

    ts, masks = args["timesteps"], args["masks"]
    x = args["img"][:N].to(F64)
    cond = sampling.pack(torch.cat((masks, args["masked_ref"]), 1)).to(F64)
    cond3 = torch.cat([cond, cond, torch.zeros_like(cond)])
    model = _stub([])
    for i, (tc, tp) in enumerate(zip(ts[:-1], ts[1:])):
        pred = model(x.repeat(3, 1, 1), cond3, torch.full((3 * N,), tc, dtype=F64), torch.full((3 * N,), 7.5, dtype=F64))
        tg, ig = sampling.get_oscillation_gs(7.5, i), sampling.get_oscillation_gs(3.0, i)
        c, u, u2 = pred.chunk(3)
        if ig > 1.0:
            upper = torch.linspace(ig, 1.0, len(ts))[i]
            ramp = torch.linspace(1.0, float(upper), _T)[None, None, :, None, None].repeat(N, 16, 1, _H, _W)
            ig = sampling.pack(ramp).to(F64)
        x = x + (tp - tc) * (u2 + ig * (u - u2) + tg * (c - u))
    return x


def test_pruned_loop_calls_the_model_on_the_branches_in_use(prune_ops):
    args = _inputs()
    pruned, batches, den = _run(args, cfg_prune=True)
    want = [N if i in (11, 13) else 3 * N for i in range(STEPS)]
    assert batches == want, batches
    assert den.last_branch_counts == [b // N for b in want]
    assert [c[1] for c in P.CALLS if c[0] == "cfg_euler_nb"] == den.last_branch_counts
    assert not [c for c in P.CALLS if c[0] == "cfg_euler"]
    unpruned, b3, den3 = _run(args, cfg_prune=False)
    assert b3 == [3 * N] * STEPS and den3.last_branch_counts == [3] * STEPS
    assert_parity(pruned, _f64_loop(args), unpruned, "pruned loop vs f64, judged against the unpruned loop (stub model)")


def test_duplicate_branches_are_detected_from_the_tensors(prune_ops):
    args = _inputs(t2v=True)
    pruned, batches, den = _run(args, cfg_prune=True)
    assert batches == [N if i in (11, 13) else 2 * N for i in range(STEPS)], batches
    unpruned, _, _ = _run(args, cfg_prune=False)
    assert_parity(pruned, _f64_loop(args), unpruned, "pruned text-to-video loop vs f64, judged against the unpruned loop (stub model)")
    # one element of the third branch's text differs: the triple is back
    other = dict(args, txt=args["txt"].clone())
    other["txt"][2 * N, 0, 0] += 1.0
    assert _run(other, cfg_prune=True)[1] == [N if i in (11, 13) else 3 * N for i in range(STEPS)]
    # ... and so it is with an image condition, whatever the prompts
    masked = dict(args, masks=args["masks"].clone())
    masked["masks"][0, 0, 0, 0, 0] = 1
    assert _run(masked, cfg_prune=True)[1] == [N if i in (11, 13) else 3 * N for i in range(STEPS)]
    ref_only = dict(args, masked_ref=args["masked_ref"].clone())
    ref_only["masked_ref"][1, 3, 1, 2, 2] = 0.5
    assert _run(ref_only, cfg_prune=True)[1] == [N if i in (11, 13) else 3 * N for i in range(STEPS)]


def test_default_path_is_the_triple_with_todays_calls(prune_ops):
    args = _inputs(t2v=True)                      # (inputs pruning WOULD act on)
    _, batches, den = _run(args)
    assert batches == [3 * N] * STEPS and den.last_branch_counts == [3] * STEPS
    assert P.CALLS == ([("copy_rows", N)] * 3 + [("cfg_euler",)]) * STEPS


def test_environment_variable_switches_pruning_on(prune_ops, monkeypatch):
    args = _inputs()
    want = [N if i in (11, 13) else 3 * N for i in range(STEPS)]
    monkeypatch.setenv("OSK_CFG_PRUNE", "1")
    assert _run(args)[1] == want
    assert _run(args, cfg_prune=False)[1] == [3 * N] * STEPS
    monkeypatch.setenv("OSK_CFG_PRUNE", "0")
    assert _run(args)[1] == [3 * N] * STEPS
    assert _run(args, cfg_prune=True)[1] == want


# ----------------------------------------------------------------------------- sequence-parallel ranks as threads
@pytest.mark.parametrize("mode", ["allgather", "ulysses"])
def test_ranks_make_the_same_plan_and_keep_their_exchange_buffers(prune_ops, mode):
    from open_sora_amd import sampling, seqpar

    ranks, name = 2, "hd64_eager_fused"
    cfg = configs.GOLDEN[name][0]
    n, T, Hh, Ww, Lt = 1, 2, 4, 6, 4                   # 12 image + 4 text tokens: 8 rows per rank, rank 0 holds image rows too
    g = torch.Generator().manual_seed(3)
    z = torch.randn(n, 16, T, Hh, Ww, generator=g).bfloat16().float()
    masks = torch.zeros(n, 1, T, Hh, Ww)
    masks[:, :, 0] = 1
    masked_ref = (torch.randn(n, 16, T, Hh, Ww, generator=g) * masks).bfloat16().float()
    txt = (torch.randn(3 * n, Lt, cfg["context_in_dim"], generator=g) * 0.2).bfloat16().float()
    y_vec = torch.randn(3 * n, cfg["vec_in_dim"], generator=g).bfloat16().float()
    img_ids, txt_ids = S.grid_ids(3 * n, T, Hh // 2, Ww // 2, Lt, torch.float32)
    ts = sampling.get_schedule(STEPS, (Hh // 2) * (Ww // 2), T)
    kw = dict(timesteps=ts, **SHIPPED)

    def inputs(dtype):
        c = lambda t: t.to(dtype)
        return dict(img=c(S.pack(z)).repeat(3, 1, 1), masks=c(masks), masked_ref=c(masked_ref), img_ids=c(img_ids), txt=c(txt),
                    txt_ids=c(txt_ids), y_vec=c(y_vec), **kw)

    model = prune_ops.Flux(device_map="cpu", torch_dtype=BF, **cfg)
    model.load_state_dict(torch_params(cfg, dtype=BF), strict=True)
    with torch.inference_mode():
        a = inputs(torch.float32)
        truth = S.i2v_denoise(S.mmdit_fn(torch_params(cfg), cfg), a.pop("img"), **a)
        single = sampling.I2VDenoiser().denoise(model, cfg_prune=True, **inputs(BF))

    def rank_fn(rank, world):
        m = copy.copy(model)
        m.forward = m.forward_ckpt
        object.__setattr__(m, "_osk_ws_cache", {})
        sp = seqpar.enable(m, mode=mode, transport=LocalTransport(world, rank, "cpu"))
        first, remade = {}, []
        cached = sp._cached

        def spy(key, make):
            b = cached(key, make)
            if first.setdefault(key, b) is not b:      # the set of this key was evicted and allocated again
                remade.append(key)
            return b

        sp._cached = spy
        den = sampling.I2VDenoiser()
        with torch.inference_mode():
            out = den.denoise(m, cfg_prune=True, **inputs(BF))
        return out.float().clone(), den.last_branch_counts, remade, len(first), len(sp._bufs)

    res = run_ranks(ranks, rank_fn, "cpu")
    want = [1 if i in (11, 13) else 3 for i in range(STEPS)]
    for out, counts, remade, n_keys, n_kept in res:
        assert counts == want
        assert not remade and n_keys == n_kept == 2 <= seqpar.SeqPar.MAX_GEOMETRIES, (remade, n_keys, n_kept)
        assert torch.equal(out, res[0][0])
        assert_parity(out, truth, single, f"pruned loop on {ranks} ranks [{mode}] vs fp32, judged against the single-rank pruned loop")


# ----------------------------------------------------------------------------- binding
def test_entry_point_is_declared_and_bound(hip_lib):
    with open(os.path.join(ROOT, "include", "osk.h")) as f:
        header = f.read()
    assert "int osk_cfg_euler_nb_bf16(const void* pred, int nb, int64_t n, const void* x, void* x_out," in header
    assert "int osk_cfg_euler_bf16(" in header and "#define OSK_ABI_VERSION 2" in header
    assert len(hip_lib.SIGNATURES["osk_cfg_euler_nb_bf16"]) == 10
    assert "osk_cfg_euler_bf16" in hip_lib.SIGNATURES and callable(hip_lib.cfg_euler_nb)
    assert hip_lib.lib.osk_abi_version() == 2
