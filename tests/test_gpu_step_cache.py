"""GPU: the sampler's step cache.  (1) osk_step_delta_bf16 (csrc/step_cache.hip) against f64 within the bound its own summation
order gives, the roll of the history buffer, bit-equal repeats; (2) osk_residual_sub_bf16 / osk_residual_add_bf16 equal to the
once-rounded f64 statement, also in the two in-place forms the sampler uses; (3) I2VDenoiser.denoise(step_cache=...) around the
small denoiser of tests/test_gpu_cfg_prune.py: threshold 0 is the plain loop bit for bit, threshold +inf skips exactly the
middle steps and meets the parity rule of tests/util.py against the rule stated on the fp32 oracle (tests/cpu_ops_step_cache.py),
judged against the CPU kernel table's run of the same loop; the same under cfg_prune; residuals kept per row; with the attention
window.  Each check prints its measured figure before it asserts (pytest -s)."""
import functools
import math

import pytest
import torch

from oracle import configs, sampling_oracle as S
from tests import cpu_ops_step_cache as P
from tests.test_gpu_mmdit import _build
from tests.test_gpu_row_kernels import assert_guards, bits, guarded
from tests.util import assert_parity, torch_params

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF = torch.bfloat16
INF = math.inf
# (B, L, C, rows of the tensor cur is a view of): one chunk; three batch items further apart than L C, partial last workgroup;
# more chunks than one pass of the 2048 x 256 grid (768000 > 524288)
SHAPES = {"one_chunk": (1, 1, 8, 1), "batch_stride": (3, 257, 1152, 300), "grid_stride": (2, 1000, 3072, 1000)}


def chain(B: int, L: int, C: int) -> int:
    """k: the longest chain of f32 roundings between an input pair and a sum of osk_step_delta_bf16, read off csrc/step_cache.hip:
    the difference (1); a lane's 8 terms per chunk, one after the other, over its ceil(chunks / (256 G)) grid-stride chunks; the
    wave butterfly (6); the four waves in order (3); in the finish a lane's ceil(G / 256) partials, butterfly (6), waves (3).
    G = min(ceil(chunks / 256), 2048) workgroups."""
    chunks = B * L * C // 8
    G = max(1, min(2048, -(-chunks // 256)))
    return 1 + 8 * -(-chunks // (256 * G)) + 6 + 3 + -(-G // 256) + 6 + 3


@functools.lru_cache(maxsize=None)
def _operands(name: str):
    """CPU bf16 (cur storage [B, rows, C], prev [B, L, C]) and the f64 sums, computed once and left unchanged"""
    B, L, C, rows = SHAPES[name]
    g = torch.Generator().manual_seed(401 + len(name))
    big = torch.randn(B, rows, C, generator=g).to(BF)
    prev = (big[:, :L].float() + 0.1 * torch.randn(B, L, C, generator=g)).to(BF)
    return big, prev, P.step_delta_f64(big[:, :L], prev)


@pytest.mark.parametrize("name", list(SHAPES))
def test_step_delta_vs_f64(hip_lib, name):
    B, L, C, rows = SHAPES[name]
    big, prev0, (num64, den64) = _operands(name)
    big_d = big.to(DEV)
    cur = big_d[:, :L]
    assert rows == L or cur.stride(0) > L * C
    flat, prev = guarded(B * L * C, BF)
    prev = prev.view(B, L, C)
    prev.copy_(prev0)
    ws = torch.empty(hip_lib.step_delta_workspace_bytes(B, L, C), dtype=torch.uint8, device=DEV)
    sums = torch.full((2,), float("nan"), device=DEV)
    hip_lib.step_delta(cur, prev, sums, ws)
    torch.cuda.synchronize()
    assert_guards(flat, B * L * C)
    assert torch.equal(bits(big_d.cpu()), bits(big)), "cur was written"
    assert torch.equal(bits(prev.cpu()), bits(big[:, :L].contiguous())), "prev is not cur bit for bit afterwards"
    k = chain(B, L, C)
    num, den = (float(v) for v in sums.double().cpu())
    e_num, e_den = abs(num - num64) / num64, abs(den - den64) / den64
    print(f"step_delta {name} {B, L, C}: rel err num {e_num:.3e} den {e_den:.3e}; allowed k 2^-24 = {k} x 2^-24 = {k * 2.0 ** -24:.3e}")
    assert e_num <= k * 2.0 ** -24 and e_den <= k * 2.0 ** -24
    # a second call on equal inputs: the same bits
    prev.copy_(prev0)
    sums2 = torch.zeros(2, device=DEV)
    hip_lib.step_delta(cur, prev, sums2, ws)
    torch.cuda.synchronize()
    assert torch.equal(bits(sums.cpu()), bits(sums2.cpu()))
    # ... and on prev == cur the distance is 0 over an unchanged denominator source
    hip_lib.step_delta(cur, prev, sums2, ws)
    torch.cuda.synchronize()
    assert float(sums2[0]) == 0.0 and float(sums2[1]) > 0.0


@pytest.mark.parametrize("name", list(SHAPES))
def test_residual_kernels_equal_the_once_rounded_f64_statement(hip_lib, name):
    B, L, C, rows = SHAPES[name]
    big, prev0, _ = _operands(name)
    a_cpu, b_cpu = big[:, :L], prev0
    big_d, b = big.to(DEV), prev0.to(DEV)
    a = big_d[:, :L]
    for fn, add in ((hip_lib.residual_sub, False), (hip_lib.residual_add, True)):
        want = P.residual_f64(a_cpu, b_cpu, add)
        flat, out = guarded(B * L * C, BF)
        out = out.view(B, L, C)
        fn(a, b, out)
        torch.cuda.synchronize()
        assert_guards(flat, B * L * C)
        wrong = int((bits(out.cpu()) != bits(want)).sum())
        print(f"residual_{'add' if add else 'sub'} {name}: {wrong} of {want.numel()} elements differ from bf16(f64)")
        assert wrong == 0
        assert torch.equal(bits(big_d.cpu()), bits(big)) and torch.equal(bits(b.cpu()), bits(prev0))
    # the sampler's in-place forms: R = Y - X over the saved X (out is b), Y = X + R over X (out is a, a strided view)
    r = b.clone()
    hip_lib.residual_sub(a, r, r)
    y = big_d.clone()
    hip_lib.residual_add(y[:, :L], b, y[:, :L])
    torch.cuda.synchronize()
    assert torch.equal(bits(r.cpu()), bits(P.residual_f64(a_cpu, b_cpu, False)))
    assert torch.equal(bits(y[:, :L].cpu()), bits(P.residual_f64(a_cpu, b_cpu, True)))
    assert torch.equal(bits(y[:, L:].cpu()), bits(big[:, L:])), "rows behind the view were written"


def test_refused_arguments_launch_nothing(hip_lib):
    cur = torch.zeros(2, 4, 32, dtype=BF, device=DEV)
    flat, prev = guarded(2 * 4 * 32, BF)
    prev = prev.view(2, 4, 32)
    sums = torch.full((2,), 7.0, device=DEV)
    ws = torch.empty(hip_lib.step_delta_workspace_bytes(2, 4, 32), dtype=torch.uint8, device=DEV)
    before = flat.clone()
    for bad in (lambda: hip_lib.step_delta(cur[:, :, 4:28], prev[:, :, :24], sums, ws),          # 8-byte aligned views, prev not contiguous
                lambda: hip_lib.step_delta(cur[:, :, 4:], prev, sums, ws),                        # shapes differ, 8-byte aligned
                lambda: hip_lib.step_delta(cur, prev, sums, ws[:4]),                              # workspace too small
                lambda: hip_lib.step_delta(cur, prev, sums.double(), ws),
                lambda: hip_lib.step_delta(cur, cur, sums, ws),                                   # overlap
                lambda: hip_lib.step_delta(cur.float(), prev, sums, ws),
                lambda: hip_lib.residual_sub(cur, prev[:1], prev),
                lambda: hip_lib.residual_add(cur[:, :, 4:12], prev[:, :, :8], prev[:, :, :8])):   # a 8-byte aligned only
        with pytest.raises(ValueError, match="osk_"):
            bad()
    torch.cuda.synchronize()
    assert torch.equal(bits(flat), bits(before)) and sums.tolist() == [7.0, 7.0]


# ----------------------------------------------------------------------------- the loop around a real small denoiser
STEPS = 14
_SHIPPED = dict(guidance=7.5, guidance_img=3.0, text_osci=True, image_osci=True, scale_temporal_osci=True)
MIDDLE_SKIPPED = [i in (0, STEPS - 1) for i in range(STEPS)]


@functools.lru_cache(maxsize=None)
def _case(Lt: int = 32):
    """the image-to-video inputs of tests/test_gpu_cfg_prune.py (CPU, bf16-representable f32), text length Lt; left unchanged"""
    from open_sora_amd import sampling

    cfg = configs.GOLDEN["hd72_eager_split"][0]
    n, T, Hh, Ww = 1, 3, 12, 8
    g = torch.Generator().manual_seed(31)
    z = torch.randn(n, 16, T, Hh, Ww, generator=g).bfloat16().float()
    masks = torch.zeros(n, 1, T, Hh, Ww)
    masks[:, :, 0] = 1
    masked_ref = (torch.randn(n, 16, T, Hh, Ww, generator=g) * masks).bfloat16().float()
    txt = (torch.randn(3 * n, Lt, cfg["context_in_dim"], generator=g) * 0.2).bfloat16().float()
    y_vec = torch.randn(3 * n, cfg["vec_in_dim"], generator=g).bfloat16().float()
    img_ids, txt_ids = S.grid_ids(3 * n, T, Hh // 2, Ww // 2, Lt, torch.float32)
    ts = sampling.get_schedule(STEPS, (Hh // 2) * (Ww // 2), T)
    tensors = dict(img=S.pack(z).repeat(3, 1, 1), masks=masks, masked_ref=masked_ref, img_ids=img_ids, txt=txt, txt_ids=txt_ids, y_vec=y_vec)
    return cfg, tensors, dict(timesteps=ts, **_SHIPPED)


def _to(tensors, dev):
    return {k: v.to(dev, BF) for k, v in tensors.items()}


@functools.lru_cache(maxsize=None)
def _references(pruned: bool):
    """(fp32 statement of the step-cached loop at threshold +inf, its record, the CPU kernel table's bf16 run of the same loop):
    computed once per schedule, shared, left unchanged"""
    from open_sora_amd import mmdit, sampling

    cfg, tensors, kw = _case()
    counts = sampling.cfg_branch_counts(STEPS, 7.5, 3.0, True, True, True, False) if pruned else [3] * STEPS
    with torch.inference_mode():
        a = dict(tensors)
        truth, record = P.i2v_denoise_step_cache(torch_params(cfg), cfg, a.pop("img"), counts=counts, threshold=INF, **a, **kw)
        hip = mmdit.ops()
        mmdit.set_ops_for_testing(P)
        try:
            model = mmdit.Flux(device_map="cpu", torch_dtype=BF, **cfg)
            model.load_state_dict(torch_params(cfg, dtype=BF), strict=True)
            emu = sampling.I2VDenoiser().denoise(model, step_cache=INF, cfg_prune=pruned, **_to(tensors, "cpu"), **kw)
        finally:
            mmdit.set_ops_for_testing(hip)
    return truth, record, emu, counts


def test_threshold_zero_is_the_plain_loop_bit_for_bit(hip_lib, monkeypatch):
    from open_sora_amd import sampling

    monkeypatch.delenv("OSK_STEP_CACHE", raising=False)
    cfg, tensors, kw = _case()
    model = _build(cfg)
    with torch.inference_mode():
        plain = sampling.I2VDenoiser().denoise(model, **_to(tensors, DEV), **kw)
        den = sampling.I2VDenoiser()
        cached = den.denoise(model, step_cache=0.0, **_to(tensors, DEV), **kw)
        torch.cuda.synchronize()
    assert torch.isfinite(plain.float()).all() and torch.equal(bits(plain), bits(cached))
    assert len(den.last_step_cache) == STEPS and all(c for _, _, c in den.last_step_cache)
    print("distances:", " ".join(f"{d:.4f}" for d, _, _ in den.last_step_cache))
    assert den.last_step_cache[0][0] == INF and all(0.0 < d < INF for d, _, _ in den.last_step_cache[1:])


@pytest.mark.parametrize("pruned", [False, True], ids=["triple", "cfg_prune"])
def test_threshold_inf_skips_the_middle_steps_and_meets_parity(hip_lib, pruned):
    """+inf skips exactly steps 1..N-2.  Under cfg_prune on the shipped oscillating schedule (3 branches, then 1 | 3 | 1 from step
    11) every row got its residual at step 0, so the per-row rule skips the one-branch step 11 too and computes the last."""
    from open_sora_amd import sampling

    cfg, tensors, kw = _case()
    truth, record, emu, counts = _references(pruned)
    model = _build(cfg)
    den = sampling.I2VDenoiser()
    with torch.inference_mode():
        out = den.denoise(model, step_cache=INF, cfg_prune=pruned, **_to(tensors, DEV), **kw)
        torch.cuda.synchronize()
    assert den.last_branch_counts == counts and (not pruned or sorted(set(counts)) == [1, 3])
    assert [c for _, _, c in den.last_step_cache] == MIDDLE_SKIPPED == [c for _, _, c in record]
    assert_parity(out, truth, emu, f"step-cached loop ({'pruned' if pruned else 'triple'}), {STEPS} steps, 2 computed, vs the fp32 statement; comparator: the CPU kernel table")


def test_pruned_loop_computes_where_a_row_has_no_residual(hip_lib, monkeypatch):
    """branch counts that START on one branch (a schedule cfg_branch_counts never makes, set here): the first step of each branch
    count is computed -- step 0, and step 2, whose rows 1 and 2 hold nothing yet -- and everything between them and the last is
    skipped, whatever its count"""
    from open_sora_amd import sampling

    counts = [1, 1, 3, 1, 3, 3, 1, 3, 1, 1, 3, 1, 3, 1]
    monkeypatch.setattr(sampling, "cfg_branch_counts", lambda *a, **k: list(counts))
    cfg, tensors, kw = _case()
    model = _build(cfg)
    den = sampling.I2VDenoiser()
    with torch.inference_mode():
        out = den.denoise(model, step_cache=INF, cfg_prune=True, **_to(tensors, DEV), **kw)
        torch.cuda.synchronize()
    assert den.last_branch_counts == counts
    assert [c for _, _, c in den.last_step_cache] == [i in (0, 2, STEPS - 1) for i in range(STEPS)]
    assert torch.isfinite(out.float()).all() and model._osk_step_cache.have == [True] * 3


def test_with_the_attention_window(hip_lib):
    from open_sora_amd import sampling

    cfg, tensors, kw = _case(64)                      # the window entry wants a text length that is a multiple of 64
    model = _build(cfg)
    with torch.inference_mode():
        plain = sampling.I2VDenoiser().denoise(model, attn_window_frames=0, **_to(tensors, DEV), **kw)
        zero = sampling.I2VDenoiser().denoise(model, attn_window_frames=0, step_cache=0.0, **_to(tensors, DEV), **kw)
        den = sampling.I2VDenoiser()
        out = den.denoise(model, attn_window_frames=0, step_cache=INF, **_to(tensors, DEV), **kw)
        torch.cuda.synchronize()
    assert torch.equal(bits(plain), bits(zero))
    assert [c for _, _, c in den.last_step_cache] == MIDDLE_SKIPPED and torch.isfinite(out.float()).all()
    assert model._attn_window is None
