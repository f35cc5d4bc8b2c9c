"""CPU: frame-window attention in fp8 mode, before a GPU is involved.  (1) The CPU statement of osk_attention_fwd_window_fp8_bf16
(tests/cpu_ops_window_fp8.py) against the f64 reference on the e4m3 operands and its derived tolerance, on every case the GPU test
runs.  (2) That tolerance can tell a wrong mask from e4m3 noise: an emulation with the table shifted by one tile, and one whose
prefix never reaches the merge, leave it -- for both fp8 kinds, on the key counts used here (every query block sees at most 64 +
484 = 548 keys; nothing had to be shrunk).  (3) A two-block MMDiT in fp8 mode with the window on runs every attention call through
the fp8 entry with n_prefix = L_txt, the table of attention_window_table and the mode of its head dim; attention_report() says so;
a kernel table without the entry keeps both refusals.  (4) Header, export, argtypes, ABI version.  The kernels themselves are
checked on the GPU by tests/test_gpu_attention_window_fp8.py, which shares the cases and the model set-up below."""
import functools
import os

import pytest
import torch

from oracle import configs
from tests import cpu_ops_window as W
from tests import cpu_ops_window_fp8 as F
from tests.util import rel_l2, torch_inputs, torch_params

BF = torch.bfloat16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = F.R
CASES = [(kind, hd, body, Bkv, table) for kind, hd in F.KIND_HD for body in F.BODIES for Bkv in (1, 2) for table in F.TABLES]


@pytest.fixture()
def fp8_window_ops(hip_lib, monkeypatch):
    from open_sora_amd import mmdit

    monkeypatch.delenv("OSK_ATTN_WINDOW_FRAMES", raising=False)
    mmdit.set_ops_for_testing(F)
    F.WINDOW_FP8_CALLS.clear()
    F.WINDOW_CALLS.clear()
    yield mmdit
    mmdit.set_ops_for_testing(hip_lib)


def packed(ops, k, v, hd, kind, device="cpu"):
    """the operands of the entry from a kernel table's own preparation calls: (k | k8, k_scale | None, vt8, v_scale)"""
    Bkv, Lk, _ = k.shape
    k, v = k.to(device), v.to(device)
    sv = ops.v_scale_fp8(v, F.H_, hd)
    vt8 = torch.zeros(Bkv, F.H_, ops.vt8_rows(hd), (Lk + 63) // 64 * 64, dtype=torch.uint8, device=device)
    ops.v_transpose_fp8(v, sv, vt8, F.H_, hd)
    if kind != "qk8":
        return k, None, vt8, sv
    sk = ops.v_scale_fp8(k, F.H_, hd)
    k8 = torch.zeros(ops.k8_shape(Bkv, F.H_, Lk, hd), dtype=torch.uint8, device=device)
    ops.k_pack_fp8(k, sk, k8, F.H_, hd)
    return k8, sk, vt8, sv


# ----------------------------------------------------------------------------- 1. the CPU statement vs f64
@pytest.mark.parametrize("kind,hd,body,Bkv,table", CASES)
def test_cpu_statement_agrees_with_the_reference(hip_lib, kind, hd, body, Bkv, table):
    q, k, v, t, ref = F.case(kind, hd, body, Bkv, table)
    kk, sk, vt8, sv = packed(F, k, v, hd, kind)
    out, lse = torch.full_like(q, float("nan")), torch.full((F.B_, F.H_, F.LQ), float("nan"))
    F.attention_fwd_window_fp8(q, kk, sk, vt8, sv, out, F.H_, hd, hd ** -0.5, n_prefix=F.NP, windows=t, mode=kind, lse=lse,
                               q_prescaled=True, kv_batches=0 if Bkv == F.B_ else Bkv, Lk=k.shape[1],
                               workspace=F.attention_window_workspace(F.B_, F.H_, F.LQ, hd, "cpu"))
    r = R.ratios(R.heads(out.float(), F.H_, hd), lse, ref)
    print(f"fp8 window CPU statement {kind} hd {hd} body {body} Bkv {Bkv} {table}: err/tol {r[0]:.3f}  dlse/tol {r[1]:.3f}")
    assert torch.isfinite(out.float()).all() and torch.isfinite(lse).all() and r[0] <= 1.0 and r[1] <= 1.0, r


def test_every_key_set_respects_the_condition_on_shapes(hip_lib):
    """what the e4m3 tolerance needs (tests/cpu_ops_window_fp8.py): at most 576 keys per query block, prefix included"""
    most = 0
    for body in F.BODIES:
        for table in F.TABLES:
            t = F.make_table(table, F.NP, body)
            assert tuple(t.shape) == (4, 2)
            hip_lib.check_window_table(t, F.LQ, F.NP + body, F.NP)
            most = max(most, max(len(F.block_keys(F.NP, F.NP + body, f_, n_)) for f_, n_ in t.tolist()))
    print("largest key set:", most)
    assert most <= F.MAX_KEYS
    hand = F.make_table("hand", F.NP, 484).tolist()
    assert hand == [[3, 1], [6, 2], [1, 5], [7, 1]] and F.make_table("hand_rev", F.NP, 484).tolist() == hand[::-1]


# ----------------------------------------------------------------------------- 2. the tolerance sees a wrong mask
@pytest.mark.parametrize("kind,hd,body,Bkv,table", [c for c in CASES if c[3] == 2])
def test_emulation_holds_and_its_mutants_leave_the_tolerance(hip_lib, kind, hd, body, Bkv, table):
    q, k, v, t, ref = F.case(kind, hd, body, Bkv, table)
    for m_mode in ("max", "max-8"):                        # the two ends of the range the running reference is allowed
        r = R.ratios(*F.emulate(q, k, v, F.H_, hd, F.NP, t, kind, m_mode), ref)
        print(f"emulation {kind} hd {hd} body {body} {table} M = {m_mode}: err/tol {r[0]:.3f}  dlse/tol {r[1]:.3f}")
        assert r[0] <= 1.0 and r[1] <= 1.0, (m_mode, r)
    tiles = (body + 63) // 64
    shifted = t.clone()
    movable = t[:, 1] < tiles                              # a full range has nowhere to go
    assert bool(movable.any())
    up = movable & (t[:, 0] + t[:, 1] < tiles)
    shifted[:, 0] += torch.where(up, 1, torch.where(movable, -1, 0)).to(torch.int32)
    for what, kw, tab in (("table shifted by one tile", {}, shifted), ("prefix dropped from the merge", dict(drop_prefix=True), t)):
        out, lse = F.emulate(q, k, v, F.H_, hd, F.NP, tab, kind, "max", **kw)
        ratio = (out.double() - ref["out"]).abs() / ref["tol"]
        print(f"{what} ({kind} hd {hd} body {body} {table}): worst err/tol {ratio.max():.2f}, {int((ratio > 1).any(-1).sum())} rows outside")
        assert ratio.max() > 1.0, what
        if not kw:                                           # every block whose range moved is caught
            for i in torch.nonzero(movable).flatten().tolist():
                assert ratio[:, :, 256 * i: 256 * (i + 1)].max() > 1.0, (what, i)


# ----------------------------------------------------------------------------- 3. the model
_T, _h, _w, _LT = 6, 8, 12, 64                              # 64 text + 6 frames x 96 image tokens: 3 query blocks, 9 image tiles
_N = _h * _w
MODELS = {72: ("hd72_eager_split", "pv8"), 128: ("hd128_liger_split", "qk8")}
QK_GAIN = 6.0      # factor on the QK-norm scale vectors: peaked attention, so that dropping keys moves the output far beyond fp8 noise


@functools.lru_cache(maxsize=None)
def model_case(hd: int):
    """(cfg, parameters, inputs) of the two-block model of this head dim, QK-norm scales raised (shared with the GPU test)"""
    cfg = dict(configs.GOLDEN[MODELS[hd][0]][0], depth=1, depth_single_blocks=1)
    params = torch_params(cfg, dtype=BF)
    for name in params:
        if name.endswith("query_norm.scale") or name.endswith("key_norm.scale"):
            params[name] = (params[name].float() * QK_GAIN).to(BF)
    return cfg, params, torch_inputs(cfg, 1, _T, _h, _w, _LT, dtype=BF)


def build(mmdit, hd: int, device="cpu"):
    cfg, params, _ = model_case(hd)
    model = mmdit.Flux(device_map=device, torch_dtype=BF, **cfg)
    model.load_state_dict({k_: v_.to(device) for k_, v_ in params.items()}, strict=True)
    return model.enable_fp8(True, qk8=True)                  # qk8 at head_dim 72 takes pv8, as the unwindowed path does


@functools.lru_cache(maxsize=None)
def cpu_forwards(hd: int):
    """(windowed W = 0, unwindowed) fp8 forwards of the model on the CPU table, f32; the caller has installed the table"""
    from open_sora_amd import mmdit

    model = build(mmdit, hd)
    x = model_case(hd)[2]
    with torch.inference_mode():
        win = model.set_attention_window(0, _N)(**x).float().clone()
        full = model.set_attention_window(None)(**x).float().clone()
    return win, full


@pytest.mark.parametrize("hd", [72, 128])
def test_fp8_model_runs_the_fp8_window_entry(fp8_window_ops, hd):
    mmdit = fp8_window_ops
    mode = MODELS[hd][1]
    model = build(mmdit, hd)
    x = model_case(hd)[2]
    assert x["txt"].shape[1] == _LT and x["img"].shape[1] == _T * _N
    with torch.inference_mode():
        full = model(**x).float().clone()
        assert not F.WINDOW_FP8_CALLS and not F.WINDOW_CALLS and model.attention_report()["attention_window"] is None
        narrow = model.set_attention_window(0, _N)(**x).float().clone()      # fp8 first, then the window
    want = tuple(map(tuple, mmdit.attention_window_table(_LT, _T * _N, _N, 0).tolist()))
    assert F.WINDOW_FP8_CALLS == [(_LT, mode, want, hd)] * 2 and not F.WINDOW_CALLS       # one double block, one single block
    rep = model.attention_report()["attention_window"]
    assert rep == {"window_frames": 0, "frame_tokens": _N, "visited_tile_fraction": pytest.approx((10 + 6 + 4) / 30), "mode": mode}
    print(f"hd {hd} {mode}: windowed (W = 0) vs unwindowed fp8 forward on the CPU table: relL2 {rel_l2(narrow, full):.3e}")
    assert torch.isfinite(narrow).all() and rel_l2(narrow, full) > 1e-2
    # the other order: the window first, then fp8; and off again is the path from before
    model.enable_fp8(False)
    model.set_attention_window(_T, _N).enable_fp8(True, qk8=True)
    F.WINDOW_FP8_CALLS.clear()
    with torch.inference_mode():
        wide = model(**x).float().clone()
        again = model.set_attention_window(None)(**x).float().clone()
    assert len(F.WINDOW_FP8_CALLS) == 2 and all(c[1] == mode and all(r == (0, 9) for r in c[2]) for c in F.WINDOW_FP8_CALLS)
    assert torch.equal(again, full)
    # W = T: every range full -- the windowed forward is the unwindowed one up to e4m3 noise (another M per launch) and the merge
    print(f"hd {hd} {mode}: W = T vs unwindowed: relL2 {rel_l2(wide, full):.3e}")
    assert rel_l2(wide, full) <= 5e-2
    # bf16 attention with the window on still reports no mode, and pv8 off means the bf16 entry
    model.enable_fp8(False).set_attention_window(1, _N)
    assert "mode" not in model.attention_report()["attention_window"]


@pytest.mark.parametrize("hd", [72, 128])
def test_the_mask_moves_the_model_far_beyond_fp8_noise(fp8_window_ops, hd):
    """The condition of the GPU end-to-end test, checked without a GPU.  That test needs sep >= 4 e_off, sep the distance between
    the windowed and the unwindowed CPU forward and e_off the HIP-vs-CPU distance with the window off, which the project's fp8
    gate holds to 5e-2: sep >= 0.2 is sufficient whatever a GPU measures inside the gate."""
    win, full = cpu_forwards(hd)
    sep = rel_l2(win, full)
    print(f"hd {hd}: the two CPU fp8 forwards are {sep:.3e} apart")
    assert torch.isfinite(win).all() and torch.isfinite(full).all() and sep >= 0.2


def test_a_table_without_the_entry_keeps_both_refusals(hip_lib, monkeypatch):
    from open_sora_amd import mmdit

    monkeypatch.delenv("OSK_ATTN_WINDOW_FRAMES", raising=False)
    assert hasattr(hip_lib, "attention_fwd_window_fp8") and not hasattr(W, "attention_fwd_window_fp8")
    mmdit.set_ops_for_testing(W)
    try:
        model = build(mmdit, 72)
        with pytest.raises(ValueError, match="fp8"):
            model.set_attention_window(1, _N)
        model.enable_fp8(False).set_attention_window(1, _N)
        with pytest.raises(ValueError, match="fp8"):
            model.enable_fp8(True)
        # a model that reached the state anyway is refused by the forward, before any launch
        for b in list(model.double_blocks) + list(model.single_blocks):
            object.__setattr__(b, "_osk_fp8", True)
        model.invalidate_plan()
        W.WINDOW_CALLS.clear()
        with torch.inference_mode(), pytest.raises(ValueError, match="fp8"):
            model(**model_case(72)[2])
        assert not W.WINDOW_CALLS
    finally:
        mmdit.set_ops_for_testing(hip_lib)
    # the library's own table has it: neither order raises
    model = build(mmdit, 72).set_attention_window(1, _N)
    assert model.enable_fp8(True)._attn_window == (1, _N)


# ----------------------------------------------------------------------------- 4. header, export, argtypes
def test_entry_point_is_declared_exported_and_bound(hip_lib):
    with open(os.path.join(ROOT, "include", "osk.h")) as f:
        header = f.read()
    assert "int osk_attention_fwd_window_fp8_bf16(const void* q, int64_t q_batch_stride, int64_t q_row_stride," in header
    assert "#define OSK_ABI_VERSION 2" in header and hip_lib.lib.osk_abi_version() == 2
    assert hasattr(hip_lib.lib, "osk_attention_fwd_window_fp8_bf16")
    # the bf16 entry's arguments, minus score_bound, plus k_scale, v_scale and mode
    assert len(hip_lib.SIGNATURES["osk_attention_fwd_window_fp8_bf16"]) == len(hip_lib.SIGNATURES["osk_attention_fwd_window_bf16"]) - 1 + 3
    assert hip_lib.ATTN_MODES == {"pv8": 1, "qk8": 2}
    for line in header.splitlines():
        if line.startswith("#define OSK_ATTN_"):
            name, value = line.split()[1:3]
            assert {"OSK_ATTN_BF16": 0, "OSK_ATTN_PV8": 1, "OSK_ATTN_QK8": 2}[name] == int(value)
    # the binding refuses a bad table and a bad mode before anything is launched (CPU tensors: a launch would fault, not raise)
    q = torch.zeros(1, 800, 256, dtype=BF)
    k = torch.zeros(1, 512, 256, dtype=BF)
    vt8 = torch.zeros(1, 2, 144, 512, dtype=torch.uint8)
    sv = torch.ones(1, 2)
    good = torch.tensor([[0, 7]] * 4, dtype=torch.int32)
    with pytest.raises(ValueError):
        hip_lib.attention_fwd_window_fp8(q, k, None, vt8, sv, torch.empty_like(q), 2, 128, 0.1, n_prefix=64, windows=good + 1, mode="pv8")
    with pytest.raises(ValueError):
        hip_lib.attention_fwd_window_fp8(q, k, None, vt8, sv, torch.empty_like(q), 2, 128, 0.1, n_prefix=64, windows=good, mode="bf16")
