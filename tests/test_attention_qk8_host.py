"""CPU: everything about the fp8-QK^T attention (head_dim 128, `qk8`) that needs no GPU -- the generator's bookkeeping for the new
loop body, the LDS image / fragment map of its 128-byte-row K tile, the argument checks of the Python wrappers, and the model's
fall-back to the pv8 attention where the kernel does not apply.  The kernel itself: tests/test_gpu_attention_qk8.py."""
import copy
import os
import re
import sys

import pytest
import torch

from oracle import configs
from tests import cpu_ops
from tests.test_lds_fragment_maps import conflicts, image_addr
from tests.util import torch_inputs, torch_params

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF = torch.bfloat16


def _gen():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_attn_asm as G
    return G


# ------------------------------------------------------------------------------------------------ generator
def test_qk8_flag_needs_head_dim_128_and_pv8():
    G = _gen()
    for hd, pv8 in ((72, True), (128, False), (72, False)):
        with pytest.raises(AssertionError):
            G.Geometry(hd, pv8=pv8, qk8=True)
    g = G.Geometry(128, pv8=True, qk8=True)
    assert (g.NKS, g.NPK, g.NPK_READ, g.KTILE, g.NKD, g.QW, g.NDT, g.RP) == (2, 4, 4, 8192, 8, 8, 5, 144)


def test_qk8_schedule_invariants():
    """MFMA counts per tile (8 QK^T + 10 P.V at NU = 2), every fragment read waited for (the generator's in-order lgkmcnt bookkeeping
    runs inside generate(), as do _check_p_ready's P-before-P.V assertions), ring depths, register ranges, <= 30 operands"""
    G = _gen()
    L = G.Layout(2, 128, pv8=True, qk8=True)
    st = G.generate(L)
    text = "\n".join(st.lines)
    assert "v_mfma_f32_32x32x16_bf16" not in text and "v_pk_" not in text
    bodies = re.split(r"\n\.L@@_body\d:", text.split("\n.L@@_rare0:")[0])[1:]
    assert len(bodies) == 2
    for k_, b in enumerate(bodies):
        mf = re.findall(r"v_mfma_f32_32x32x64_f8f6f4 (\w)\[", b)
        assert mf.count("v") == 8 and mf.count("a") == 10, mf       # scores go to VGPRs, O^T accumulates in AGPRs
        assert b.count("ds_read_b128") == 2 * 4 + 2 * 5              # 4 K fragments + 5 V^T fragments of two reads each
        assert b.count("global_load_lds_dwordx4") == L.NSLOT + L.NSLOT_V == 5 and b.count("s_barrier") == 1
        assert b.count("v_exp_f32") == 64 and b.count("v_cvt_pk_fp8_f32") == 32 and b.count("v_fma_f32") == 64
        assert "v_cndmask" not in b                                   # no clamped K offsets: the packed K repeats the last key
        # P ready before the first P.V of the body's own tile: every pack sits in front of the first accumulating MFMA behind the entry
        own = b.split(".L@@_entry%d:" % k_)[1]
        first_pv = re.search(r"v_mfma_f32_32x32x64_f8f6f4 a\[", own).start()
        assert own[:first_pv].count("v_cvt_pk_fp8_f32") == 32
        # the dequantisation FMAs and the max chains read scores only after the last QK^T MFMA that writes them has been issued
        last_qk = [m.end() for m in re.finditer(r"v_mfma_f32_32x32x64_f8f6f4 v\[", own)][-1]
        assert "v_fma_f32" not in own[:last_qk] and "v_max" not in own[:last_qk]
    # prologue 8 QK^T + per body (2 trailing + 8 + 8) + exit 2 trailing
    assert len(re.findall(r"v_mfma_f32_32x32x64_f8f6f4 v\[", text)) == 3 * 8
    assert len(re.findall(r"v_mfma_f32_32x32x64_f8f6f4 a\[", text)) == 2 * 10 + 2
    # ring depths: K fragments alternate between two 8-register slots, V^T fragments likewise
    kdst = re.findall(r"v_mfma_f32_32x32x64_f8f6f4 v\[\d+:\d+\], v\[(\d+):(\d+)\], a\[(\d+):(\d+)\]", bodies[0])
    assert [int(a) for a, _, _, _ in kdst] == [L.KR0, L.KR0, L.KR0 + 8, L.KR0 + 8] * 2
    assert {(int(a), int(b)) for _, _, a, b in kdst} == {(160 + 8 * i, 167 + 8 * i) for i in range(4)}
    assert L.KRD == 2 and L.RD == 2 and L.A_END == 192
    for m in re.finditer(r"\bv(\d+)\b", text):
        assert L.V_FIRST <= int(m.group(1)) < L.V_END, m.group(0)
    for m in re.finditer(r"\bv\[(\d+):(\d+)\]", text):
        assert L.V_FIRST <= int(m.group(1)) and int(m.group(2)) < L.V_END, m.group(0)
    for m in re.finditer(r"\ba\[(\d+):(\d+)\]", text):
        assert int(m.group(2)) < L.A_END
    for m in re.finditer(r"\bs(\d+)\b", text):
        assert G.S_FIRST <= int(m.group(1)) <= G.S_LAST, m.group(0)
    assert len(L.OPERANDS) <= 30 and "koffL0" not in L.OPERANDS and {"c0", "c1"} <= set(L.OPERANDS)
    assert L.V_END <= 256 and L.V_END + L.A_END <= 512
    for m in re.finditer(r"ds_read_b128 [^\n]* offset:(\d+)", text):
        assert int(m.group(1)) < 65536
    assert L.G.SMEM == 2 * 8192 + 2 * 144 * 64


def test_qk8_rare_path_rescales_o_and_shifts_the_pending_scores():
    G = _gen()
    L = G.Layout(2, 128, pv8=True, qk8=True)
    text = "\n".join(G.generate(L).lines)
    rare = text.split("\n.L@@_rare0:")[1].split("\n.L@@_rare1:")[0]
    assert rare.count("v_add_f32") == 2 * (1 + 32) + 2          # per block: M + d, the 32 pending scores; plus M_old - M_new
    assert rare.count("v_mul_f32") == 160 and rare.count("v_accvgpr_write_b32") == 160   # O^T only: no Q padding dim to rewrite


# ------------------------------------------------------------------------------------------------ LDS image of the K tile
def _k_frag_addr(lane, ks, j, t2):
    """address the lane reads with read j (0, 1) of fragment (ks, t2): key row 32 t2 + l % 32, logical chunk 4 ks + 2 (l / 32) + j"""
    return image_addr(32 * t2 + (lane & 31), 4 * ks + 2 * (lane >> 5) + j)


def test_k8_fragment_reads_cover_the_tile_exactly_once():
    seen = {}
    for ks in range(2):
        for t2 in range(2):
            for j in range(2):
                for lane in range(64):
                    a = _k_frag_addr(lane, ks, j, t2)
                    row, pos = a // 128, (a % 128) // 16
                    chunk = pos ^ ((row >> 1) & 7)
                    for byte in range(16):
                        key = (row, chunk * 16 + byte)
                        assert key not in seen
                        # the operand layout: register (4 j + byte / 4) of lane (l31, hi) holds dims 64 ks + 32 hi + 16 j + byte
                        assert key == (32 * t2 + (lane & 31), 64 * ks + 32 * (lane >> 5) + 16 * j + byte)
                        seen[key] = 1
    assert len(seen) == 64 * 128


@pytest.mark.parametrize("ks", range(2))
@pytest.mark.parametrize("j", range(2))
@pytest.mark.parametrize("t2", range(2))
def test_k8_fragment_reads_are_conflict_free(ks, j, t2):
    assert conflicts(lambda l: _k_frag_addr(l, ks, j, t2)) == 0
    # every 16-byte slot of the 256-byte bank window is hit by exactly one lane of each 16-lane group: all banks equally
    from tests.test_lds_fragment_maps import GROUPS
    for g in GROUPS:
        assert sorted((_k_frag_addr(l, ks, j, t2) >> 4) & 15 for l in g) == list(range(16))


def test_k8_unswizzled_rows_would_conflict():
    assert conflicts(lambda l: (l & 31) * 128 + ((2 * (l >> 5)) << 4)) > 0


def test_k8_lds_dma_pieces_write_whole_swizzled_rows():
    """instruction j = wave + 4 i of the K loader covers key rows 8 j .. 8 j + 7 (the wrapper's koff): lane l lands at row l / 8,
    position l % 8, and fetches bytes 16 ((l % 8) ^ key) .. of that row of the packed K"""
    seen = set()
    for wave in range(4):
        for i in range(2):
            j = wave + 4 * i
            for l in range(64):
                row = 8 * j + (l >> 3)
                src = row * 128 + (((l & 7) ^ ((row >> 1) & 7)) << 4)         # koff[i] of the wrapper
                chunk = (src % 128) >> 4
                assert src // 128 == row and image_addr(row, chunk) == j * 1024 + l * 16
                seen.add((row, chunk))
    assert len(seen) == 64 * 8


# ------------------------------------------------------------------------------------------------ wrappers
def _wrapper_args(hip_lib, B=1, H=2, Lq=70, Lk=65):
    D = H * 128
    Lp = (Lk + 63) // 64 * 64
    return dict(q=torch.zeros(B, Lq, D, dtype=BF), k8=torch.zeros(B, H, Lp, 128, dtype=torch.uint8),
                ks=torch.ones(B, H), vt8=torch.zeros(B, H, hip_lib.vt8_rows(128), Lp, dtype=torch.uint8), vs=torch.ones(B, H),
                out=torch.zeros(B, Lq, D, dtype=BF), H=H, Lk=Lk)


def _no_launch(hip_lib, monkeypatch):
    class Refuse:
        def __getattr__(self, name):
            raise RuntimeError("the wrapper reached the library: " + name)
    monkeypatch.setattr(hip_lib, "lib", Refuse())


def test_attention_fwd_qk8_wrapper_checks_before_any_launch(hip_lib, monkeypatch):
    _no_launch(hip_lib, monkeypatch)
    a = _wrapper_args(hip_lib)
    call = lambda hd=128, **kw: hip_lib.attention_fwd_qk8(*[{**a, **kw}[n] for n in ("q", "k8", "ks", "vt8", "vs", "out")], a["H"], hd,
                                                          hd ** -0.5, seg_len=a["Lk"])
    with pytest.raises(AssertionError):
        call(k8=a["k8"].to(torch.int8))                                    # wrong dtype
    with pytest.raises(AssertionError):
        call(q=a["q"].float())
    with pytest.raises(AssertionError):
        call(q=torch.zeros(1, 70, 512, dtype=BF)[:, :, ::2])               # non-contiguous last dim
    with pytest.raises(AssertionError):
        call(k8=torch.zeros(1, 2, 128, 256, dtype=torch.uint8)[:, :, :, ::2])
    with pytest.raises(AssertionError, match="head_dim 128"):
        call(hd=72)
    with pytest.raises(AssertionError):
        call(ks=torch.ones(1, 3))                                          # one scale per (key batch, head)
    with pytest.raises(RuntimeError, match="reached the library"):         # a well-formed call does get there
        call()


def test_k_pack_fp8_wrapper_checks_before_any_launch(hip_lib, monkeypatch):
    _no_launch(hip_lib, monkeypatch)
    B, H, L = 2, 2, 65
    k = torch.zeros(B, L, H * 128, dtype=BF)
    s = torch.ones(B, H)
    k8 = torch.zeros(hip_lib.k8_shape(B, H, L), dtype=torch.uint8)
    assert hip_lib.k8_shape(B, H, L) == (B, H, 128, 128)
    with pytest.raises(AssertionError):
        hip_lib.k_pack_fp8(k.float(), s, k8, H, 128)
    with pytest.raises(AssertionError):
        hip_lib.k_pack_fp8(torch.zeros(B, L, 2 * H * 128, dtype=BF)[:, :, ::2], s, k8, H, 128)
    with pytest.raises(AssertionError, match="head_dim 128"):
        hip_lib.k_pack_fp8(torch.zeros(B, L, H * 72, dtype=BF), s, k8, H, 72)
    with pytest.raises(AssertionError):
        hip_lib.k_pack_fp8(k, s, k8[:, :, :64], H, 128)                    # rows not padded to the tile
    with pytest.raises(RuntimeError, match="reached the library"):
        hip_lib.k_pack_fp8(k, s, k8, H, 128)


def test_c_abi_declares_the_two_entries(hip_lib):
    hdr = open(os.path.join(ROOT, "include", "osk.h")).read()
    for name in ("osk_k_pack_fp8", "osk_attention_fwd_qk8_bf16"):
        assert name in hip_lib.SIGNATURES and re.search(r"\bint %s\(" % name, hdr)
    assert "#define OSK_ABI_VERSION 2" in hdr or hip_lib.lib.osk_abi_version() == 2


# ------------------------------------------------------------------------------------------------ model
class _Ops:
    """the CPU emulation of the kernels, with the qk8 entries recorded and served by the pv8 emulation on the unpacked K"""

    def __init__(self):
        self.n_pv8 = self.n_qk8 = 0
        self._k = {}

    def __getattr__(self, name):
        return getattr(cpu_ops, name)

    def attention_fwd_pv8(self, *a, **kw):
        self.n_pv8 += 1
        return cpu_ops.attention_fwd_pv8(*a, **kw)

    def k8_shape(self, B, H, L, hd=128):
        assert hd == 128
        return (B, H, (L + 63) // 64 * 64, 128)

    def k_pack_fp8(self, k, scales, k8, H, hd):
        assert hd == 128 and tuple(k8.shape) == self.k8_shape(k.shape[0], H, k.shape[1]) and scales.shape == (k.shape[0], H)
        self._k[k8.data_ptr()] = k
        return k8

    def attention_fwd_qk8(self, q, k8, k_scale, vt8, v_scale, out, H, hd, scale, *, seg_len, **kw):
        self.n_qk8 += 1
        k = self._k[k8.data_ptr()]
        assert seg_len == k.shape[1]
        return cpu_ops.attention_fwd_pv8(q, k, vt8, v_scale, out, H, hd, scale, **kw)


@pytest.fixture()
def ops_mmdit(hip_lib):
    from open_sora_amd import mmdit

    ops = _Ops()
    mmdit.set_ops_for_testing(ops)
    yield mmdit, ops
    mmdit.set_ops_for_testing(hip_lib)


def _model(mmdit, cfg):
    model = mmdit.Flux(device_map="cpu", torch_dtype=BF, **cfg)
    model.load_state_dict(torch_params(cfg, dtype=BF), strict=True)
    return model


def test_enable_fp8_qk8_selects_the_new_entry_at_head_dim_128_only(ops_mmdit):
    mmdit, ops = ops_mmdit
    cfg = dict(configs.GOLDEN["hd128_eager_fused"][0], depth=1, depth_single_blocks=1)
    model = _model(mmdit, cfg)
    inp = torch_inputs(cfg, 2, 2, 12, 12, 160, dtype=BF)
    with torch.inference_mode():
        ref16 = model(**inp).clone()
        model.enable_fp8()(**inp)
        assert (ops.n_pv8, ops.n_qk8) == (2, 0)                       # the present arguments select what they select today
        model.enable_fp8(qk8=True)(**inp)
        assert (ops.n_pv8, ops.n_qk8) == (2, 2)
        assert all(p.qk8 and p.pv8 for p in [mmdit.plan_double(model.double_blocks[0]), mmdit.plan_single(model.single_blocks[0])])
        again16 = model.enable_fp8(False)(**inp).clone()
    assert (ops.n_pv8, ops.n_qk8) == (2, 2) and torch.equal(again16, ref16)
    assert not mmdit.plan_double(model.double_blocks[0]).qk8

    cfg72 = dict(configs.GOLDEN["hd72_eager_split"][0], depth=1, depth_single_blocks=1)
    m72 = _model(mmdit, cfg72)
    ops.n_pv8 = ops.n_qk8 = 0
    with torch.inference_mode():
        m72.enable_fp8(qk8=True)(**torch_inputs(cfg72, 2, 2, 12, 12, 160, dtype=BF))
    assert ops.n_pv8 == 2 and ops.n_qk8 == 0                          # head_dim 72: today's pv8 path, silently


@pytest.mark.parametrize("mode", ["allgather", "ulysses"])
def test_enable_fp8_qk8_keeps_pv8_under_sequence_parallelism(ops_mmdit, mode):
    from open_sora_amd import seqpar
    from tests.local_transport import LocalTransport, run_ranks

    mmdit, ops = ops_mmdit
    cfg = dict(configs.GOLDEN["hd128_eager_fused"][0], depth=1, depth_single_blocks=1)
    model = _model(mmdit, cfg).enable_fp8(qk8=True)
    inp = torch_inputs(cfg, 2, 2, 2, 4, 4, dtype=BF)

    def rank_fn(rank, world):
        m = copy.copy(model)
        m.forward = m.forward_ckpt
        object.__setattr__(m, "_osk_ws_cache", {})
        seqpar.enable(m, mode=mode, transport=LocalTransport(world, rank, "cpu"))
        with torch.inference_mode():
            return m(**inp).float().clone()

    res = run_ranks(2, rank_fn, "cpu")
    assert torch.equal(res[0], res[1])
    assert ops.n_qk8 == 0 and ops.n_pv8 == 2 * 2                      # two blocks on two ranks
