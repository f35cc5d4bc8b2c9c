"""CPU test of the f64 references of the row kernels (tests/cpu_ops_rows_f64.py) -- runs without a GPU.

Each reference is compared with the project's f32 oracle (oracle/mmdit_oracle.py) on the inputs of tests/test_gpu_row_kernels.py,
through the very check_* functions that file applies to the kernels' outputs.  A tolerance that the oracle's own f32 arithmetic
did not fit would fail here first, so the GPU tolerances admit the reference implementation's arithmetic and nothing looser.
Every check prints its measured figure (pytest -s).
"""
import pytest
import torch
import torch.nn.functional as F

from oracle import mmdit_oracle as O
from tests import cpu_ops_rows_f64 as R
from tests import row_kernel_cases as RC
from tests.cpu_ops import pos2key


# ----------------------------------------------------------------------------- LayerNorm + modulate
def _oracle_ln(c):
    return ((1 + c["scale"][:, None]) * O._layer_norm(c["x"].float()) + c["shift"][:, None]).bfloat16()


@pytest.mark.parametrize("D", RC.LN_D)
def test_ln_modulate_reference_vs_oracle(D):
    c = RC.ln_case(D)
    RC.check_ln(_oracle_ln(c), c)


@pytest.mark.parametrize("D", RC.LN_D)
def test_ln_modulate_fp8_reference_vs_oracle_and_tie_share(D):
    """the oracle path in place of the kernel: f32 LayerNorm + modulate -> bf16 -> the row quantiser.  Also the proof that the
    chosen seeds keep the reference's own tie share under the 0.5 % cap."""
    c = RC.ln_case(D)
    q, s = R.quantize_rows_e4m3(_oracle_ln(c).reshape(-1, D))
    RC.check_ln_fp8(q, s, c)


def test_bf16_tie_mask_finds_the_ties():
    y = torch.tensor([1.0 + 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -20, 1.0 + 2.0 ** -8 + 2.0 ** -30, 1.0, 1.0 - 2.0 ** -9 - 2.0 ** -30,
                      1.0 - 2.0 ** -9 - 2.0 ** -20, -(2.5 + 2.0 ** -7 - 2.0 ** -31), 0.3], dtype=torch.float64)
    m = R.bf16_tie_mask(y, torch.full_like(y, 2.0 ** -25))
    assert m.tolist() == [True, False, True, False, True, False, True, False]
    assert R.e4m3_ordinal(torch.tensor([0x00, 0x80, 0x01, 0x81, 0x7E, 0xFE], dtype=torch.uint8)).tolist() == [0, 0, 1, -1, 126, -126]


# ----------------------------------------------------------------------------- QK-RMSNorm + RoPE
def _oracle_qk(c, name):
    B, L, H, hd, D = c["B"], c["L"], c["H"], c["hd"], c["D"]
    t = "qk".index(name)
    x0 = c["big"][:, 1: L + 1, 8 + t * D: 8 + (t + 1) * D].reshape(B, L, H, hd).permute(0, 2, 1, 3)
    ls = c["l_split"]
    n = torch.cat([O.rms_norm(x0[:, :, :ls], c["scales"][t]), O.rms_norm(x0[:, :, ls:], c["scales"][2 + t])], 2)
    rope = O.apply_rope_half if c["mode"] == 1 else O.apply_rope_interleaved
    if name == "q" and c["q_mult"] != 1.0:
        o = (rope(n.float(), c["ang"]) * c["q_mult"]).bfloat16()      # rotate in f32, scale in f32, ONE rounding
    else:
        o = rope(n, c["ang"])                                         # bf16 tensors -> the reference's rounding points
    return o.permute(0, 2, 1, 3).reshape(B, L, D)


@pytest.mark.parametrize("H,hd,mode,variant", RC.qk_case_ids())
def test_qknorm_rope_reference_vs_oracle(H, hd, mode, variant):
    c = RC.qk_case(H, hd, mode, variant)
    for name in c["which"]:
        RC.check_qk(_oracle_qk(c, name), c, name)


# ----------------------------------------------------------------------------- V transpose
@pytest.mark.parametrize("hd", [64, 72, 128])
def test_vt_key_order_equals_pos2key(hd):
    for Lp in (64, 128, 192):
        order = R.vt_key_order(hd, Lp)
        assert torch.equal(order, pos2key(hd, Lp))
        assert sorted(order.tolist()) == list(range(Lp))            # a permutation: every key stored exactly once
    for L in RC.VT_L:
        c = RC.vt_case(hd, L)
        B, H, Lp = RC.VT_B, RC.VT_H, c["Lp"]
        vpad = torch.zeros(B, Lp, H, hd, dtype=torch.bfloat16)
        vpad[:, :L] = c["v"].reshape(B, L, H, hd)
        assert torch.equal(c["ref"], vpad[:, pos2key(hd, Lp)].permute(0, 2, 3, 1))


# ----------------------------------------------------------------------------- GEMV
@pytest.mark.parametrize("Bv,K,act_in", RC.GEMV_CASES)
def test_gemv_reference_vs_oracle(Bv, K, act_in):
    c = RC.gemv_case(Bv, K, act_in)
    xin = F.silu(c["x"]) if act_in else c["x"]
    got = torch.zeros(Bv, c["ncol"])
    for (w, b), c0 in zip(c["layers"], c["cols"]):
        sd = {"l.weight": w.float()}
        if b is not None:
            sd["l.bias"] = b.float()
        got[:, c0: c0 + w.shape[0]] = O._lin(sd, "l", xin)           # the oracle's Linear (Modulation: _lin(silu(vec)))
    RC.check_gemv(got, c)
    RC.check_gemv(got + got, c, units=2)


# ----------------------------------------------------------------------------- timestep embedding, RoPE tables
@pytest.mark.parametrize("B,dim,tf,mp", RC.TE_CASES)
def test_timestep_embedding_reference_vs_oracle(B, dim, tf, mp):
    c = RC.te_case(B, dim, tf, mp)
    emb = O.timestep_embedding(c["t"], dim, max_period=mp, time_factor=tf)   # (no zero column for an odd dim: layers.py pads it)
    got = torch.zeros(B, dim)
    got[:, : 2 * (dim // 2)] = emb
    RC.check_te(got, c)
    if dim % 2:
        assert bool((c["ref"][:, -1] == 0).all())


@pytest.mark.parametrize("n_axes", [1, 2, 3, 4])
def test_rope_table_reference_vs_oracle(n_axes):
    c = RC.rope_case(n_axes)
    ang = O.rope_angles(c["ids"][None], c["axes"], RC.QK_THETA)[0]
    RC.check_rope(torch.cos(ang).float(), torch.sin(ang).float(), c, False)
    a32 = O.rope_angles_liger(c["ids"][None], c["axes"], RC.QK_THETA)[0]
    assert a32.dtype == torch.float32
    RC.check_rope(torch.cos(a32), torch.sin(a32), c, True)
    assert float(c["ids"].max()) >= 4000.0 and c["half"] * RC.ROPE_ROWS > 256


# ----------------------------------------------------------------------------- CFG + Euler, row copy
@pytest.mark.parametrize("name", list(RC.CFG_CASES))
def test_cfg_euler_reference_vs_f32(name):
    c = RC.cfg_case(name)
    cond, u, u2 = c["pred"].float()
    g = c["g"] if c["g"] is not None else RC.CFG_G_IMG
    got = (c["x"].float() + RC.CFG_DT * (u2 + g * (u - u2) + RC.CFG_G_TXT * (cond - u))).bfloat16()
    RC.check_cfg(got, c)


def test_copy_rows_reference():
    src = RC.rnd("cp.s", (3, 1, 5, 8))
    dst = RC.rnd("cp.d", (3, 2, 5, 12))
    out = R.copy_rows_ref(src, dst)
    assert torch.equal(out[..., :8], src.expand(3, 2, 5, 8)) and torch.equal(out[..., 8:], dst[..., 8:])
