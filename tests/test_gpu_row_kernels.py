"""GPU tests of the row kernels of the denoise step (csrc/elementwise.hip): every host-side dispatch class, class edge and tail
of LayerNorm + modulate (bf16 and fp8), QK-RMSNorm + RoPE (row-per-thread and lane-group kernels), V transpose, the GEMV task
list, timestep embedding, RoPE tables, CFG + Euler and the strided row copy, against the plain f64 references of
tests/cpu_ops_rows_f64.py.

Cases, seeded inputs, expectations and the acceptance checks live in tests/row_kernel_cases.py; tests/test_row_kernel_refs.py
runs the same checks on the f32 oracle without a GPU, which is where the tolerances are settled.  Conventions here: every
output lies inside a larger sentinel-filled buffer (guard rows, guard columns, guard bands before and after) that must come back
bit for bit; every output element is compared; in-place and LDS-staged kernels run three times on fresh copies and must agree
bit for bit; each check prints its measured figure before it asserts (pytest -s).

What reaches which dispatch path (ids as pytest prints them):
  ln_modulate, bf16 and fp8   MAXC 1 / 2 / 3 / 4 / 6 / 8 and both sides of every class edge: [D8_MAXC1] .. [D4096_MAXC8]; refused D: [4104], [12], [516]
  qknorm, rows kernel NT 128  H 4, 5, 7, 16, 24, 64, 65, 100, 128 x hd 64, 72 x both modes: [H-hd-mode-base]
  qknorm, rows kernel NT 256  H 129, 256;  lane-group kernel: H 3, 257, hd 128 ([3-128-*], [24-128-*])
  qknorm call shapes          H 4, 6, 24, 129 x hd 72, 64 x both modes: [..-q_only], [..-k_only], [..-csb0], [..-lsplit0], [..-lsplitL], [..-qmult],
                              [..-unaligned], [..-unaligned_qmult], [..-csb_odd] (fallback to the lane-group kernel, same inputs and
                              expectation as [..-base] / [..-qmult]), [..-rows] (all-zero and x300-outlier rows), [..-seqpar_k], [..-seqpar_q]
                              (one-sided, shared table, softmax scale), [..-few_tokens] (B L below one block)
  v_transpose                 L 1, 63, 64, 65, 150 x hd 64, 72, 128, guard bands around V^T
  gemv_tasks                  [9-2048-*] slices 8 + 1, [3-2048-1] one 4-row slice, [5-2056-1] / [5-4096-*] slices 4 + 1, [2-4104-*], [*-16384-*] 1-row
                              slices, [*-8-*] one chunk; act_in 0 and 1; layers of 1, 3, 4, 5, 7, 8, 9, 64, 65, 100 rows; strided x / out; refused K
  timestep_embedding          odd dim, time_factor 1 and 37.5, max_period 1000, several blocks
  rope_table                  1 - 4 axes x f64 / f32 angles, positions up to ~ 5e3; refused: odd widths, five axes
  cfg_euler                   [vec], [one_chunk], [in_place], [in_place_vec], [grid_stride]
  copy_rows                   [tokens_to_chunks], [chunks_to_tokens], grid_stride
"""
import pytest
import torch

from tests import cpu_ops_rows_f64 as R
from tests import row_kernel_cases as RC

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF = torch.bfloat16
_INT = {1: torch.uint8, 2: torch.int16, 4: torch.int32}
_SENTINEL = {1: 0xA5, 2: 0x7BCD, 4: 0x7B3C1234}   # bf16 ~ 2.1e36, f32 ~ 9.8e35: finite, and nothing a kernel would compute


def bits(t: torch.Tensor) -> torch.Tensor:
    return t.view(_INT[t.element_size()])


def sentinel(shape, dtype) -> torch.Tensor:
    size = torch.empty((), dtype=dtype).element_size()
    return torch.full(tuple(shape), _SENTINEL[size], dtype=_INT[size], device=DEV).view(dtype)


def guarded(n: int, dtype, guard: int = 64):
    """(flat sentinel buffer of guard + n + guard elements, its n inner elements)"""
    flat = sentinel((n + 2 * guard,), dtype)
    return flat, flat[guard: guard + n]


def assert_guards(flat: torch.Tensor, n: int, guard: int = 64) -> None:
    want = _SENTINEL[flat.element_size()]
    assert bool((bits(flat[:guard]) == want).all()) and bool((bits(flat[guard + n:]) == want).all()), "wrote outside the destination"


def assert_rest_untouched(after: torch.Tensor, before: torch.Tensor, *written) -> None:
    """after == before bit for bit outside the index tuples in `written`"""
    a, b = bits(after).clone(), bits(before).clone()
    for idx in written:
        a[idx] = 0
        b[idx] = 0
    assert torch.equal(a, b), "wrote outside the destination"


def assert_all_equal(outs) -> None:
    for o in outs[1:]:
        assert torch.equal(bits(outs[0]), bits(o)), "two runs on the same input differ"


ALL = slice(None)


# ----------------------------------------------------------------------------- LayerNorm + modulate
def _ln_operands(c):
    B, L, D = c["B"], c["L"], c["D"]
    x = c["xbuf"].to(DEV)[:, 2: 2 + L, 8: 8 + D]
    mod = c["mod"].to(DEV)
    return x, mod, mod[:, :D], mod[:, D + 8: 2 * D + 8]


@pytest.mark.parametrize("D", RC.LN_D, ids=[f"D{d}_MAXC{RC.LN_MAXC[d]}" for d in RC.LN_D])
def test_ln_modulate_every_class_and_edge(hip_lib, D):
    c = RC.ln_case(D)
    B, L = c["B"], c["L"]
    x, mod, shift, scale = _ln_operands(c)
    big = sentinel((B, L + 2, D + 16), BF)
    before = big.clone()
    out = big[:, 1: L + 1, 8: 8 + D]
    hip_lib.ln_modulate(x, shift, scale, out, mod.stride(0))
    torch.cuda.synchronize()
    assert_rest_untouched(big, before, (ALL, slice(1, L + 1), slice(8, 8 + D)))
    RC.check_ln(out.cpu(), c)


@pytest.mark.parametrize("D", RC.LN_D, ids=[f"D{d}_MAXC{RC.LN_MAXC[d]}" for d in RC.LN_D])
def test_ln_modulate_fp8_vs_independent_reference(hip_lib, D):
    c = RC.ln_case(D)
    B, L = c["B"], c["L"]
    M = B * L
    x, mod, shift, scale = _ln_operands(c)
    flat8, out8 = guarded(M * D, torch.uint8)
    flats, scales = guarded(M, torch.float32, 16)
    rc = hip_lib.lib.osk_ln_modulate_fp8(x.data_ptr(), x.stride(0), x.stride(1), out8.data_ptr(), scales.data_ptr(), shift.data_ptr(),
                                         scale.data_ptr(), mod.stride(0), B, L, D, 1e-6, hip_lib._stream())
    assert rc == 0
    torch.cuda.synchronize()
    assert_guards(flat8, M * D)
    assert_guards(flats, M, 16)
    RC.check_ln_fp8(out8.view(M, D).cpu(), scales.cpu(), c)


@pytest.mark.parametrize("D", RC.LN_REFUSED_D)
def test_ln_modulate_refuses_and_writes_nothing(hip_lib, D):
    """D past 8 chunks of 8 per lane, or no multiple of 8: refused by both entry points, nothing launched.  Every stride and
    pointer is valid (a multiple of 8 elements), so D alone is what is refused."""
    B, L = 2, 5
    Dp = (D + 7) // 8 * 8 + 16
    x = RC.rnd("ln.refused", (B, L, Dp)).to(DEV)[:, :, :D]
    mod = RC.rnd("ln.refused.mod", (B, 2 * Dp), dtype=torch.float32).to(DEV)
    shift, scale = mod[:, :D], mod[:, Dp: Dp + D]
    big = sentinel((B, L, Dp), BF)
    with pytest.raises(RuntimeError):
        hip_lib.ln_modulate(x, shift, scale, big[:, :, :D], mod.stride(0))
    flat8, out8 = guarded(B * L * D, torch.uint8)
    flats, scales = guarded(B * L, torch.float32, 16)
    rc = hip_lib.lib.osk_ln_modulate_fp8(x.data_ptr(), x.stride(0), x.stride(1), out8.data_ptr(), scales.data_ptr(), shift.data_ptr(),
                                         scale.data_ptr(), mod.stride(0), B, L, D, 1e-6, hip_lib._stream())
    assert rc < 0
    torch.cuda.synchronize()
    for t in (big, flat8, flats):
        assert bool((bits(t) == _SENTINEL[t.element_size()]).all())


# ----------------------------------------------------------------------------- QK-RMSNorm + RoPE
def _qk_tables_on_device(c):
    """(cos, sin, batch stride) on the device.  `unaligned`: the tables start one float past a 16-byte boundary; `csb_pad`: their
    batch stride is no multiple of 4 floats.  Either way the row-per-thread kernel cannot read them with its 16-byte pieces and the
    host falls back to the lane-group kernel."""
    Bt, L, half = c["cos"].shape
    stride = L * half + c["csb_pad"]
    off = 1 if c["unaligned"] else 0
    out = []
    for t in (c["cos"], c["sin"]):
        flat = torch.zeros(off + Bt * stride + 8, dtype=torch.float32, device=DEV)
        view = flat.as_strided((Bt, L, half), (stride, half, 1), off)
        view.copy_(t)
        assert view.data_ptr() % 16 == 4 * off
        out.append(view)
    csb = 0 if c["csb0"] else stride
    assert c["csb_pad"] or csb % 4 == 0       # (so that only what the variant names decides between the two kernels)
    return out[0], out[1], csb


@pytest.mark.parametrize("H,hd,mode,variant", RC.qk_case_ids())
def test_qknorm_rope_every_head_count_and_call_shape(hip_lib, H, hd, mode, variant):
    """in place on the q / k columns of the fused [B, L, 3 D] projection output: the V columns, the other tensor of a one-sided
    call and the guard rows / columns around the buffer are the sentinel"""
    c = RC.qk_case(H, hd, mode, variant)
    B, L, D = c["B"], c["L"], c["D"]
    big0 = c["big"].to(DEV)
    scales = [s.to(DEV) for s in c["scales"]]
    cos, sin, csb = _qk_tables_on_device(c)
    runs = []
    for _ in range(3):
        big = big0.clone()
        y = big[:, 1: L + 1, 8: 8 + 3 * D]
        q = y[:, :, :D] if "q" in c["which"] else None
        k = y[:, :, D: 2 * D] if "k" in c["which"] else None
        hip_lib.qknorm_rope(q, k, scales[0], scales[1], scales[2], scales[3], c["l_split"], cos, sin, csb, H, hd, mode, q_mult=c["q_mult"])
        runs.append(big)
    torch.cuda.synchronize()
    assert_all_equal(runs)
    cols = {"q": slice(8, 8 + D), "k": slice(8 + D, 8 + 2 * D)}
    assert_rest_untouched(runs[0], big0, *[(ALL, slice(1, L + 1), cols[n]) for n in c["which"]])
    got = runs[0].cpu()
    for n in c["which"]:
        RC.check_qk(got[:, 1: L + 1, cols[n]], c, n)


# ----------------------------------------------------------------------------- V transpose (bit exact)
@pytest.mark.parametrize("L", RC.VT_L)
@pytest.mark.parametrize("hd", [64, 72, 128])
def test_v_transpose_tails_and_guard_bands(hip_lib, hd, L):
    c = RC.vt_case(hd, L)
    B, H, Lp = RC.VT_B, RC.VT_H, c["Lp"]
    D = H * hd
    v = c["y"].to(DEV)[:, :, 2 * D:]
    n = B * H * hd * Lp
    runs = []
    for _ in range(3):
        flat, inner = guarded(n, BF, 512)
        hip_lib.v_transpose(v, inner.view(B, H, hd, Lp), H, hd)
        runs.append(flat)
    torch.cuda.synchronize()
    assert_all_equal(runs)
    assert_guards(runs[0], n, 512)
    assert torch.equal(bits(runs[0][512: 512 + n].view(B, H, hd, Lp).cpu()), bits(c["ref"]))


# ----------------------------------------------------------------------------- GEMV task list
@pytest.mark.parametrize("Bv,K,act_in", RC.GEMV_CASES)
def test_gemv_tasks_slices_edges_and_row_counts(hip_lib, Bv, K, act_in):
    c = RC.gemv_case(Bv, K, act_in)
    ncol = c["ncol"]
    x = c["xbuf"].to(DEV)[:, :K]
    layers = [(w.to(DEV), None if b is None else b.to(DEV), col) for (w, b), col in zip(c["layers"], c["cols"])]
    tasks = hip_lib.GemvTasks(layers, DEV)
    runs = []
    for _ in range(3):
        big = sentinel((Bv + 2, ncol + 16), torch.float32)
        hip_lib.gemv_tasks(x, tasks, big[1: Bv + 1, 8: 8 + ncol], act_in=act_in)
        runs.append(big)
    torch.cuda.synchronize()
    assert_all_equal(runs)
    cov = torch.nonzero(c["covered"]).flatten().to(DEV) + 8
    assert_rest_untouched(runs[0], sentinel(runs[0].shape, torch.float32), (slice(1, Bv + 1), cov))
    RC.check_gemv(runs[0][1: Bv + 1, 8: 8 + ncol].cpu(), c)
    hip_lib.gemv_tasks(x, tasks, runs[1][1: Bv + 1, 8: 8 + ncol], act_in=act_in, accumulate=True)
    torch.cuda.synchronize()
    assert_rest_untouched(runs[1], sentinel(runs[1].shape, torch.float32), (slice(1, Bv + 1), cov))
    RC.check_gemv(runs[1][1: Bv + 1, 8: 8 + ncol].cpu(), c, units=2)


@pytest.mark.parametrize("K", RC.GEMV_REFUSED_K)
def test_gemv_tasks_refuses_and_writes_nothing(hip_lib, K):
    """one x row past 64 KiB of LDS, or K no multiple of 8"""
    x = RC.rnd("gv.refused", (2, K), dtype=torch.float32).to(DEV)
    tasks = hip_lib.GemvTasks([(RC.rnd("gv.refused.w", (4, K)).to(DEV), None, 0)], DEV)
    out = sentinel((2, 8), torch.float32)
    with pytest.raises(RuntimeError):
        hip_lib.gemv_tasks(x, tasks, out, act_in=1)
    torch.cuda.synchronize()
    assert bool((bits(out) == _SENTINEL[4]).all())


# ----------------------------------------------------------------------------- timestep embedding, RoPE tables
@pytest.mark.parametrize("B,dim,tf,mp", RC.TE_CASES)
def test_timestep_embedding_odd_dims_and_factors(hip_lib, B, dim, tf, mp):
    c = RC.te_case(B, dim, tf, mp)
    flat, inner = guarded(B * dim, torch.float32, 16)
    hip_lib.timestep_embedding(c["t"].to(DEV), inner.view(B, dim), max_period=mp, time_factor=tf)
    torch.cuda.synchronize()
    assert_guards(flat, B * dim, 16)
    RC.check_te(inner.view(B, dim).cpu(), c)


@pytest.mark.parametrize("f32_angles", [False, True], ids=["f64_angles", "f32_angles"])
@pytest.mark.parametrize("n_axes", [1, 2, 3, 4])
def test_rope_table_axis_counts_and_large_positions(hip_lib, n_axes, f32_angles):
    """the f64-angle tables keep the flat 2e-5; with f32 angles the allowance grows with |angle| * f32 epsilon (row_kernel_cases)"""
    c = RC.rope_case(n_axes)
    n = RC.ROPE_ROWS * c["half"]
    fc, cos = guarded(n, torch.float32, 16)
    fs, sin = guarded(n, torch.float32, 16)
    hip_lib.rope_table(c["ids"].to(DEV), c["axes"], RC.QK_THETA, f32_angles, cos, sin)
    torch.cuda.synchronize()
    assert_guards(fc, n, 16)
    assert_guards(fs, n, 16)
    RC.check_rope(cos.view(RC.ROPE_ROWS, c["half"]).cpu(), sin.view(RC.ROPE_ROWS, c["half"]).cpu(), c, f32_angles)


@pytest.mark.parametrize("axes", RC.ROPE_REFUSED_AXES, ids=lambda a: "x".join(map(str, a)))
def test_rope_table_refuses_odd_widths_and_a_fifth_axis(hip_lib, axes):
    ids = torch.zeros(4, len(axes), dtype=torch.float32, device=DEV)
    cos, sin = sentinel((4 * 64,), torch.float32), sentinel((4 * 64,), torch.float32)
    with pytest.raises(RuntimeError):
        hip_lib.rope_table(ids, axes, RC.QK_THETA, False, cos, sin)
    torch.cuda.synchronize()
    assert bool((bits(cos) == _SENTINEL[4]).all()) and bool((bits(sin) == _SENTINEL[4]).all())


# ----------------------------------------------------------------------------- CFG + Euler
@pytest.mark.parametrize("name", list(RC.CFG_CASES))
def test_cfg_euler_vector_guidance_in_place_and_grid_stride(hip_lib, name):
    c = RC.cfg_case(name)
    n = c["n"]
    if name == "grid_stride":
        assert n > RC.CFG_GRID
    pred = c["pred"].to(DEV)
    g = None if c["g"] is None else c["g"].to(DEV)
    flat, out = guarded(n, BF)
    if c["in_place"]:
        out.copy_(c["x"])
        x = out
    else:
        x = c["x"].to(DEV)
    hip_lib.cfg_euler(pred, x, out, RC.CFG_G_TXT, RC.CFG_G_IMG, RC.CFG_DT, g_img_vec=g)
    torch.cuda.synchronize()
    assert_guards(flat, n)
    if not c["in_place"]:
        assert torch.equal(bits(x.cpu()), bits(c["x"]))
    RC.check_cfg(out.cpu(), c)


# ----------------------------------------------------------------------------- strided row copy (bit exact)
@pytest.mark.parametrize("direction", ["tokens_to_chunks", "chunks_to_tokens"])
def test_copy_rows_chunked_rearrangement_both_ways(hip_lib, direction):
    """the sequence-parallel rearrangement: [B, L, P x Dg] (chunk j = columns j Dg ..) <-> [P, B, L, Dg], each side a view inside a
    wider buffer, so chunk, batch and row strides all differ between the two sides"""
    B, L, P, Dg = 2, 37, 3, 68
    tok_shape, chk_shape = (B, L + 2, P * Dg + 8), (P, B, L + 2, Dg + 8)

    def tok_view(big):
        return big[:, 1: L + 1, 4: 4 + P * Dg].unflatten(2, (P, Dg)).permute(2, 0, 1, 3)

    def chk_view(big):
        return big[:, :, 1: L + 1, 4: 4 + Dg]

    if direction == "tokens_to_chunks":
        src_big, dst_big, src_view, dst_view = RC.rnd("cp.tok", tok_shape, seed=271).to(DEV), sentinel(chk_shape, BF), tok_view, chk_view
    else:
        src_big, dst_big, src_view, dst_view = RC.rnd("cp.chk", chk_shape, seed=272).to(DEV), sentinel(tok_shape, BF), chk_view, tok_view
    src, dst = src_view(src_big), dst_view(dst_big)
    assert src.stride(0) != dst.stride(0) and src.stride(1) != dst.stride(1) and src.stride(2) != dst.stride(2)
    want_big = dst_big.cpu().clone()
    dst_view(want_big).copy_(R.copy_rows_ref(src.cpu(), dst_view(dst_big.cpu())))
    hip_lib.copy_rows(src, dst)
    torch.cuda.synchronize()
    assert torch.equal(bits(dst_big.cpu()), bits(want_big))


def test_copy_rows_grid_stride(hip_lib):
    """more 8-byte units than one pass of the full grid covers (4096 blocks x 256 threads)"""
    L, C = 4100, 1024
    assert L * (C // 4) > RC.COPY_GRID
    src = RC.rnd("cp.big", (1, L, C), seed=273).to(DEV)
    dst_big = sentinel((1, L + 2, C + 8), BF)
    want_big = dst_big.cpu().clone()
    want_big[:, 1: L + 1, 4: 4 + C] = R.copy_rows_ref(src.cpu(), want_big[:, 1: L + 1, 4: 4 + C])
    hip_lib.copy_rows(src, dst_big[:, 1: L + 1, 4: 4 + C])
    torch.cuda.synchronize()
    assert torch.equal(bits(dst_big.cpu()), bits(want_big))
