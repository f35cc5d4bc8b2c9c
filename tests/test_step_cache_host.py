"""CPU: the host side of the sampler's step cache (I2VDenoiser.denoise(step_cache=...), open_sora_amd/sampling.py): the decision
rule as a pure function, keyword and environment parsing, the loop around a real small denoiser on the CPU kernel table
(tests/cpu_ops_step_cache.py) against the rule stated on the fp32 oracle, the three refusals, and the bindings' argument
validation.  The kernels themselves are checked on the GPU by tests/test_gpu_step_cache.py."""
import math
import os

import pytest
import torch

from oracle import configs, sampling_oracle as S
from tests import cpu_ops_step_cache as P
from tests.util import torch_params

BF = torch.bfloat16
INF = math.inf
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIPPED = dict(guidance=7.5, guidance_img=3.0, text_osci=True, image_osci=True, scale_temporal_osci=True)


# ----------------------------------------------------------------------------- the decision rule
def _walk(ds, threshold, coefficients=None, have=None):
    """the decisions of a whole loop: [(computed, acc carried on)]"""
    from open_sora_amd.sampling import step_cache_decide

    acc, out = 0.0, []
    for i, d in enumerate(ds):
        computed, acc = step_cache_decide(i, len(ds), d, acc, threshold, coefficients, True if have is None else have[i])
        out.append((computed, acc))
    return out


def test_first_and_last_step_are_computed_whatever_the_distance():
    got = _walk([0.0, 0.0, 0.0, 0.0], INF)
    assert [c for c, _ in got] == [True, False, False, True]
    assert got[0][1] == 0.0 and got[-1][1] == 0.0
    assert [c for c, _ in _walk([0.0], INF)] == [True]
    assert [c for c, _ in _walk([0.0, 0.0], INF)] == [True, True]


def test_accumulation_and_the_reset_after_a_computed_step():
    # acc: 0.25, 0.5 (both < 0.6: skipped), 0.75 -> computed and reset, 0.25 skipped, last forced
    got = _walk([9.0, 0.25, 0.25, 0.25, 0.25, 9.0], 0.6)
    assert got == [(True, 0.0), (False, 0.25), (False, 0.5), (True, 0.0), (False, 0.25), (True, 0.0)]
    # the comparison is strict: acc == threshold computes
    assert _walk([0.0, 0.5, 0.0], 0.5)[1] == (True, 0.0)
    # threshold 0 never skips (acc >= 0 under the identity), +inf skips every middle step with a finite distance
    assert all(c for c, _ in _walk([0.0] * 6, 0.0))
    assert [c for c, _ in _walk([1e30] * 6, INF)] == [True, False, False, False, False, True]


def test_infinite_or_nan_distance_computes():
    assert _walk([0.0, INF, 0.0, 0.0], INF) == [(True, 0.0), (True, 0.0), (False, 0.0), (True, 0.0)]
    assert _walk([0.0, float("nan"), 0.0, 0.0], INF)[1] == (True, 0.0)
    assert _walk([0.0, INF, 0.0, 0.0], 1.0)[1:3] == [(True, 0.0), (False, 0.0)]


def test_a_missing_residual_forces_a_compute():
    got = _walk([0.0, 0.1, 0.1, 0.1, 0.0], 10.0, have=[False, True, False, True, True])
    assert got == [(True, 0.0), (False, 0.1), (True, 0.0), (False, 0.1), (True, 0.0)]


def test_polynomial_evaluation_highest_power_first():
    from open_sora_amd.sampling import step_cache_decide, step_cache_poly

    assert step_cache_poly(None, 0.375) == 0.375 and step_cache_poly([1, 0], 0.375) == 0.375
    assert step_cache_poly([2.0, -3.0, 0.5], 2.0) == 2.0 * 4 - 3.0 * 2 + 0.5
    assert step_cache_poly([4.0], 123.0) == 4.0
    assert step_cache_poly([], 5.0) == 0.0
    # the decision uses it: 2 d^2 at d = 0.5 adds 0.5
    assert step_cache_decide(1, 4, 0.5, 0.25, 1.0, [2.0, 0.0, 0.0]) == (False, 0.75)
    assert step_cache_decide(2, 4, 0.5, 0.75, 1.0, [2.0, 0.0, 0.0]) == (True, 0.0)


# ----------------------------------------------------------------------------- the loop on the CPU kernel table
STEPS = 8
_N, _T, _H, _W, _LT = 1, 2, 4, 6, 4


@pytest.fixture()
def sc_ops(hip_lib, monkeypatch):
    from open_sora_amd import mmdit

    for k in ("OSK_STEP_CACHE", "OSK_CFG_PRUNE", "OSK_ATTN_WINDOW_FRAMES"):
        monkeypatch.delenv(k, raising=False)
    mmdit.set_ops_for_testing(P)
    P.CALLS.clear()
    yield mmdit
    mmdit.set_ops_for_testing(hip_lib)


def _case(steps=STEPS):
    from open_sora_amd import sampling

    cfg = configs.GOLDEN["hd64_eager_fused"][0]
    n, T, Hh, Ww, Lt = _N, _T, _H, _W, _LT
    g = torch.Generator().manual_seed(11)
    z = torch.randn(n, 16, T, Hh, Ww, generator=g).bfloat16().float()
    masks = torch.zeros(n, 1, T, Hh, Ww)
    masks[:, :, 0] = 1
    masked_ref = (torch.randn(n, 16, T, Hh, Ww, generator=g) * masks).bfloat16().float()
    txt = (torch.randn(3 * n, Lt, cfg["context_in_dim"], generator=g) * 0.2).bfloat16().float()
    y_vec = torch.randn(3 * n, cfg["vec_in_dim"], generator=g).bfloat16().float()
    img_ids, txt_ids = S.grid_ids(3 * n, T, Hh // 2, Ww // 2, Lt, torch.float32)
    ts = sampling.get_schedule(steps, (Hh // 2) * (Ww // 2), T)
    tensors = dict(img=S.pack(z).repeat(3, 1, 1), masks=masks, masked_ref=masked_ref, img_ids=img_ids, txt=txt, txt_ids=txt_ids, y_vec=y_vec)
    return cfg, tensors, dict(timesteps=ts, **SHIPPED)


def _model(mmdit, cfg):
    model = mmdit.Flux(device_map="cpu", torch_dtype=BF, **cfg)
    model.load_state_dict(torch_params(cfg, dtype=BF), strict=True)
    return model


def _bf(tensors):
    return {k: v.to(BF) for k, v in tensors.items()}


def test_threshold_zero_is_the_plain_loop_bit_for_bit(sc_ops):
    from open_sora_amd import sampling

    cfg, tensors, kw = _case()
    model = _model(sc_ops, cfg)
    with torch.inference_mode():
        plain = sampling.I2VDenoiser().denoise(model, **_bf(tensors), **kw)
        den = sampling.I2VDenoiser()
        cached = den.denoise(model, step_cache=0.0, **_bf(tensors), **kw)
    assert torch.equal(plain, cached)
    assert len(den.last_step_cache) == STEPS and all(c for _, _, c in den.last_step_cache)
    assert den.last_step_cache[0][0] == INF and all(0.0 < d < INF for d, _, _ in den.last_step_cache[1:])
    assert [c[0] for c in P.CALLS].count("residual_add") == 0 and [c[0] for c in P.CALLS].count("residual_sub") == STEPS


def test_threshold_inf_skips_every_middle_step_and_follows_the_rule(sc_ops):
    from open_sora_amd import sampling

    cfg, tensors, kw = _case()
    model = _model(sc_ops, cfg)
    with torch.inference_mode():
        den = sampling.I2VDenoiser()
        cached = den.denoise(model, step_cache=INF, **_bf(tensors), **kw)
        a = dict(tensors)
        truth, record = P.i2v_denoise_step_cache(torch_params(cfg), cfg, a.pop("img"), counts=[3] * STEPS, threshold=INF, **a, **kw)
        plain = sampling.I2VDenoiser().denoise(model, **_bf(tensors), **kw)
        a = dict(tensors)
        plain_truth = S.i2v_denoise(S.mmdit_fn(torch_params(cfg), cfg), a.pop("img"), **a, **kw)
    want = [i in (0, STEPS - 1) for i in range(STEPS)]
    assert [c for _, _, c in den.last_step_cache] == want == [c for _, _, c in record]
    assert [c[0] for c in P.CALLS if c[0].startswith("residual")][:STEPS] == ["residual_sub"] + ["residual_add"] * (STEPS - 2) + ["residual_sub"]
    for (d, _, _), (d_ref, _, _) in list(zip(den.last_step_cache, record))[1:]:
        assert d == pytest.approx(d_ref, rel=0.1), (d, d_ref)     # bf16 M against fp32 M: the distance is a difference of near-equal rows
    # comparator: how far the bf16 emulation of the PLAIN loop is from the plain fp32 loop
    e_plain = float((plain.float() - plain_truth).norm() / plain_truth.norm())
    e_cached = float((cached.float() - truth).norm() / truth.norm())
    print(f"step-cached loop vs its fp32 statement: relL2 {e_cached:.3e}; plain loop vs its fp32 statement: {e_plain:.3e}")
    assert e_cached <= max(1.5 * e_plain, 2.0 ** -8)
    assert not torch.equal(cached, plain)                             # skipping changes the result


def test_pruned_loop_keeps_residuals_per_row(sc_ops, monkeypatch):
    """counts that start on ONE branch: the first three-branch step finds rows 1 and 2 without a residual and must compute"""
    from open_sora_amd import sampling

    counts = [1, 1, 3, 1, 3, 3, 1, 3]
    monkeypatch.setattr(sampling, "cfg_branch_counts", lambda *a, **k: list(counts))
    cfg, tensors, kw = _case()
    model = _model(sc_ops, cfg)
    with torch.inference_mode():
        den = sampling.I2VDenoiser()
        cached = den.denoise(model, step_cache=INF, cfg_prune=True, **_bf(tensors), **kw)
        a = dict(tensors)
        truth, record = P.i2v_denoise_step_cache(torch_params(cfg), cfg, a.pop("img"), counts=counts, threshold=INF, **a, **kw)
    assert den.last_branch_counts == counts
    assert [c for _, _, c in den.last_step_cache] == [True, False, True, False, False, False, False, True] == [c for _, _, c in record]
    # rows of every residual call: stored for 1 row at step 0, for all 3 at step 2 (rows 1, 2 were missing) and at the last step
    assert [c for c in P.CALLS if c[0].startswith("residual")] == [("residual_sub", 1), ("residual_add", 1), ("residual_sub", 3), ("residual_add", 1),
                                                                  ("residual_add", 3), ("residual_add", 3), ("residual_add", 1), ("residual_sub", 3)]
    assert [c for c in P.CALLS if c[0] == "step_delta"] == [("step_delta", 1)] * STEPS        # the conditional rows only, every step
    assert torch.isfinite(cached.float()).all() and torch.isfinite(truth).all()


# ----------------------------------------------------------------------------- keyword and environment
def _spy_loop(monkeypatch):
    """replaces the three loops by recorders: which one denoise() picks, and with which threshold / coefficients"""
    from open_sora_amd import sampling

    seen = []

    def cached(*a):
        seen.append(("step_cache", a[-3], a[-2]))
        return a[2]

    monkeypatch.setattr(sampling.I2VDenoiser, "_loop_step_cache", staticmethod(cached))
    monkeypatch.setattr(sampling.I2VDenoiser, "_loop", staticmethod(lambda *a: seen.append(("plain",)) or a[2]))
    monkeypatch.setattr(sampling.I2VDenoiser, "_loop_pruned", staticmethod(lambda *a: seen.append(("pruned",)) or a[2]))
    return seen


def test_keyword_and_environment_parsing(sc_ops, monkeypatch):
    from open_sora_amd import sampling

    cfg, tensors, kw = _case()
    model = _model(sc_ops, cfg)
    seen = _spy_loop(monkeypatch)
    run = lambda **extra: sampling.I2VDenoiser().denoise(model, **_bf(tensors), **kw, **extra)
    run()
    run(step_cache=None)
    run(step_cache=0.25, step_cache_coefficients=(3, 2, 1))
    run(step_cache=0)
    monkeypatch.setenv("OSK_STEP_CACHE", "0.125")
    run()
    run(step_cache=None)                     # the keyword wins: off
    run(step_cache=2)
    monkeypatch.setenv("OSK_STEP_CACHE", " ")
    run()
    monkeypatch.setenv("OSK_STEP_CACHE", "inf")
    run(cfg_prune=True)
    assert seen == [("plain",), ("plain",), ("step_cache", 0.25, [3.0, 2.0, 1.0]), ("step_cache", 0.0, None), ("step_cache", 0.125, None),
                    ("plain",), ("step_cache", 2.0, None), ("plain",), ("step_cache", INF, None)]
    monkeypatch.setenv("OSK_STEP_CACHE", "often")
    with pytest.raises(ValueError):
        run()


# ----------------------------------------------------------------------------- the three refusals
def test_refused_with_hip_graph(sc_ops):
    from open_sora_amd import sampling

    cfg, tensors, kw = _case()
    with pytest.raises(ValueError, match="hip_graph"):
        sampling.I2VDenoiser().denoise(_model(sc_ops, cfg), step_cache=0.1, hip_graph=True, **_bf(tensors), **kw)


def test_refused_under_sequence_parallelism(sc_ops):
    from open_sora_amd import sampling

    cfg, tensors, kw = _case()
    model = _model(sc_ops, cfg)
    model._sp = object()                      # what seqpar.enable leaves on the model
    with pytest.raises(ValueError, match="sequence parallelism"):
        sampling.I2VDenoiser().denoise(model, step_cache=0.1, **_bf(tensors), **kw)
    with pytest.raises(ValueError, match="sequence parallelism"):
        model.step_cache_begin(1, 3, 12, "cpu")


def test_refused_for_models_without_the_split(sc_ops):
    from open_sora_amd import sampling

    cfg, tensors, kw = _case()
    calls = []
    foreign = lambda **k: calls.append(1)
    with pytest.raises(ValueError, match="split"):
        sampling.I2VDenoiser().denoise(foreign, step_cache=0.1, **_bf(tensors), **kw)
    with pytest.raises(ValueError, match="DistilledDenoiser"):
        sampling.DistilledDenoiser().denoise(foreign, img=tensors["img"][:1], timesteps=kw["timesteps"], guidance=4.0, step_cache=0.1)
    assert not calls


# ----------------------------------------------------------------------------- bindings
def test_bindings_are_declared_and_validate_before_any_launch(hip_lib):
    with open(os.path.join(ROOT, "include", "osk.h")) as f:
        header = f.read()
    for name in ("osk_step_delta_bf16", "osk_step_delta_workspace_bytes", "osk_residual_sub_bf16", "osk_residual_add_bf16"):
        assert f" {name}(" in header and name in hip_lib.SIGNATURES
    assert "#define OSK_ABI_VERSION 2" in header and hip_lib.lib.osk_abi_version() == 2
    assert hip_lib.step_delta_workspace_bytes(1, 1, 8) == 8
    assert hip_lib.step_delta_workspace_bytes(2, 1000, 3072) == 8 * 2048
    assert hip_lib.step_delta_workspace_bytes(3, 257, 1152) == 8 * ((3 * 257 * 144 + 255) // 256)
    cur, prev = torch.zeros(1, 4, 16, dtype=BF), torch.zeros(1, 4, 16, dtype=BF)
    sums, ws = torch.zeros(2), torch.zeros(64, dtype=torch.uint8)
    with pytest.raises(ValueError, match="osk_step_delta_bf16"):
        hip_lib.step_delta(cur, prev, sums, ws)                      # CPU tensors
    with pytest.raises(ValueError, match="osk_residual_sub_bf16"):
        hip_lib.residual_sub(cur, prev, prev)
    with pytest.raises(ValueError, match="osk_residual_add_bf16"):
        hip_lib.residual_add(cur, prev, cur)
    # the library refuses what the binding would have refused too: status < 0, nothing launched
    lib = hip_lib.lib
    assert lib.osk_step_delta_bf16(None, 16, 16, 0x1000, 0x2000, 1, 1, 16, 0x3000, 8, None) < 0
    assert lib.osk_step_delta_bf16(0x1000, 16, 16, 0x2000, 0x3000, 1, 1, 12, 0x4000, 8, None) < 0        # C % 8
    assert lib.osk_step_delta_bf16(0x1000, 16, 16, 0x2000, 0x3000, 1, 1, 16, 0x4000, 4, None) < 0        # workspace too small
    assert lib.osk_step_delta_bf16(0x1008, 16, 16, 0x2000, 0x3000, 1, 1, 16, 0x4000, 8, None) < 0        # alignment
    assert lib.osk_step_delta_bf16(0x1000, 16, 12, 0x2000, 0x3000, 1, 2, 16, 0x4000, 8, None) < 0        # row stride
    assert lib.osk_residual_sub_bf16(0x1000, 16, 16, None, 16, 16, 0x2000, 16, 16, 1, 1, 16, None) < 0
    assert lib.osk_residual_add_bf16(0x1000, 16, 16, 0x2000, 16, 16, 0x3000, 16, 16, 1, 1, 20, None) < 0
