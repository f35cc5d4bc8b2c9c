"""GPU: CFG branch pruning.  (1) osk_cfg_euler_nb_bf16 (csrc/elementwise.hip) for 1, 2 and 3 branches against the f64 reference
of tests/cpu_ops_cfg_prune.py with the tolerances of the existing combine kernel (tests/row_kernel_cases.py), inside sentinel
guards, with the chunks a branch count does not use set to NaN; bit equality with osk_cfg_euler_bf16 at three branches; refused
arguments.  (2) I2VDenoiser.denoise(cfg_prune=True) around a real small denoiser, image-to-video and text-to-video, against the
fp32 CPU oracle loop and judged against the unpruned loop of the same model; with hip_graph=True bit for bit the eager pruned run.
Each check prints its measured figure before it asserts (pytest -s)."""
import functools

import pytest
import torch

from oracle import configs, sampling_oracle as S
from tests import cpu_ops_cfg_prune as P
from tests import row_kernel_cases as RC
from tests.test_gpu_kernels import bf16_ulp_close
from tests.test_gpu_mmdit import _build
from tests.test_gpu_row_kernels import assert_guards, bits, guarded, sentinel
from tests.util import assert_parity, torch_params

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF = torch.bfloat16
NAN = float("nan")
# one chunk of 8; a partial second block (257 chunks of 8, 256 per block); one chunk past a full pass of the 2048 x 256 grid
SIZES = {"one_chunk": 8, "second_block": 8 * 257, "grid_stride": 8 * (2048 * 256 + 1)}


@functools.lru_cache(maxsize=1)
def _operands(n: int):
    """CPU inputs of size n, shared by the branch counts (left unchanged): pred [3, n], x [n], per-element g_img [n]"""
    return (RC.rnd("cfgnb.p", (3, n), seed=271), RC.rnd("cfgnb.x", (n,), seed=272),
            RC.rnd("cfgnb.g", (n,), std=1.0, mean=3.0, seed=273, dtype=torch.float32))


@functools.lru_cache(maxsize=3)
def _expected(n: int, nb: int, vec: bool):
    pred, x, g = _operands(n)
    return P.cfg_euler_nb_f64(pred, nb, x, RC.CFG_G_TXT, g if vec else RC.CFG_G_IMG, RC.CFG_DT)


def _device_pred(pred: torch.Tensor, nb: int) -> torch.Tensor:
    """[3, n] on the device, the chunks behind the nb in use set to NaN: a kernel that read them would not return finite numbers"""
    p = pred.to(DEV)
    p[nb:] = NAN
    return p


def _check(got: torch.Tensor, ref: torch.Tensor, what: str) -> None:
    assert bool(torch.isfinite(got.float()).all()), f"{what}: non-finite output (a chunk behind the branches in use was read)"
    print(f"{what}: abs term needed {RC.excess(got, ref, RC.CFG_REL):.3e} (allowed {RC.CFG_ABS:.0e})")
    bf16_ulp_close(got.double(), ref, rel=RC.CFG_REL, abs_=RC.CFG_ABS)


@pytest.mark.parametrize("vec", [False, True], ids=["scalar", "vec"])
@pytest.mark.parametrize("nb", [1, 2, 3])
@pytest.mark.parametrize("size", list(SIZES))
def test_cfg_euler_nb_vs_f64(hip_lib, size, nb, vec):
    n = SIZES[size]
    pred, x, g = _operands(n)
    p, xd = _device_pred(pred, nb), x.to(DEV)
    # below three branches the image guidance is not an operand: NaN there must not reach the output either
    gd = None if not vec else (g.to(DEV) if nb == 3 else torch.full((n,), NAN, device=DEV))
    g_img = RC.CFG_G_IMG if nb == 3 else NAN
    flat, out = guarded(n, BF)
    hip_lib.cfg_euler_nb(p, nb, xd, out, RC.CFG_G_TXT, g_img, RC.CFG_DT, g_img_vec=gd)
    torch.cuda.synchronize()
    assert_guards(flat, n)
    assert torch.equal(bits(xd.cpu()), bits(x))
    _check(out.cpu(), _expected(n, nb, vec), f"cfg_euler_nb nb={nb} n={n} {'vec' if vec else 'scalar'}")


def test_cfg_euler_nb_in_place(hip_lib):
    n, nb = SIZES["second_block"], 2
    pred, x, _ = _operands(n)
    flat, out = guarded(n, BF)
    out.copy_(x)
    hip_lib.cfg_euler_nb(_device_pred(pred, nb), nb, out, out, RC.CFG_G_TXT, RC.CFG_G_IMG, RC.CFG_DT)
    torch.cuda.synchronize()
    assert_guards(flat, n)
    _check(out.cpu(), _expected(n, nb, False), f"cfg_euler_nb in place nb={nb} n={n}")


@pytest.mark.parametrize("vec", [False, True], ids=["scalar", "vec"])
@pytest.mark.parametrize("size", ["second_block", "grid_stride"])
def test_three_branches_are_the_existing_kernel_bit_for_bit(hip_lib, size, vec):
    n = SIZES[size]
    pred, x, g = _operands(n)
    p, xd, gd = pred.to(DEV), x.to(DEV), (g.to(DEV) if vec else None)
    a, b = torch.empty(n, dtype=BF, device=DEV), torch.empty(n, dtype=BF, device=DEV)
    hip_lib.cfg_euler(p, xd, a, RC.CFG_G_TXT, RC.CFG_G_IMG, RC.CFG_DT, g_img_vec=gd)
    hip_lib.cfg_euler_nb(p, 3, xd, b, RC.CFG_G_TXT, RC.CFG_G_IMG, RC.CFG_DT, g_img_vec=gd)
    torch.cuda.synchronize()
    assert torch.equal(bits(a), bits(b))


@pytest.mark.parametrize("nb,n", [(0, 64), (4, 64), (2, 60)], ids=["nb0", "nb4", "n_not_multiple_of_8"])
def test_refused_arguments_launch_nothing(hip_lib, nb, n):
    pred = torch.zeros(4, 64, dtype=BF, device=DEV)
    x = torch.zeros(64, dtype=BF, device=DEV)[:n]
    flat, out = guarded(n, BF)
    with pytest.raises(RuntimeError, match="osk_cfg_euler_nb_bf16"):
        hip_lib.cfg_euler_nb(pred, nb, x, out, 7.5, 3.0, -0.05)
    assert hip_lib.lib.osk_cfg_euler_nb_bf16(None, 2, 64, x.data_ptr(), out.data_ptr(), 7.5, 3.0, None, -0.05, None) < 0
    torch.cuda.synchronize()
    assert bool((bits(flat) == bits(sentinel((1,), BF))).all())


# ----------------------------------------------------------------------------- the loop around a real small denoiser
STEPS = 14
_N, _T, _H, _W, _LT = 1, 3, 12, 8, 32
_SHIPPED = dict(guidance=7.5, guidance_img=3.0, text_osci=True, image_osci=True, scale_temporal_osci=True)


@functools.lru_cache(maxsize=None)
def _case(t2v: bool):
    """inputs (CPU, bf16-representable f32) and the fp32 oracle loop's result, computed once and left unchanged"""
    from open_sora_amd import sampling

    cfg = configs.GOLDEN["hd72_eager_split"][0]
    n, T, Hh, Ww, Lt = _N, _T, _H, _W, _LT
    g = torch.Generator().manual_seed(31 + t2v)
    z = torch.randn(n, 16, T, Hh, Ww, generator=g).bfloat16().float()
    masks = torch.zeros(n, 1, T, Hh, Ww)
    if not t2v:
        masks[:, :, 0] = 1
    masked_ref = (torch.randn(n, 16, T, Hh, Ww, generator=g) * masks).bfloat16().float()
    txt = (torch.randn(3 * n, Lt, cfg["context_in_dim"], generator=g) * 0.2).bfloat16().float()
    y_vec = torch.randn(3 * n, cfg["vec_in_dim"], generator=g).bfloat16().float()
    if t2v:                                                  # prepare_guidance: text + neg + neg
        txt[2 * n:] = txt[n:2 * n]
        y_vec[2 * n:] = y_vec[n:2 * n]
    img_ids, txt_ids = S.grid_ids(3 * n, T, Hh // 2, Ww // 2, Lt, torch.float32)
    ts = sampling.get_schedule(STEPS, (Hh // 2) * (Ww // 2), T)
    tensors = dict(img=S.pack(z).repeat(3, 1, 1), masks=masks, masked_ref=masked_ref, img_ids=img_ids, txt=txt, txt_ids=txt_ids,
                   y_vec=y_vec)
    kw = dict(timesteps=ts, **_SHIPPED)
    with torch.inference_mode():
        a = dict(tensors)
        truth = S.i2v_denoise(S.mmdit_fn(torch_params(cfg), cfg), a.pop("img"), **a, **kw)
    return cfg, tensors, kw, truth


def _args(t2v: bool):
    cfg, tensors, kw, truth = _case(t2v)
    return cfg, dict({k: v.to(DEV, BF) for k, v in tensors.items()}, **kw), truth


@pytest.mark.parametrize("t2v", [False, True], ids=["image_to_video", "text_to_video"])
def test_pruned_loop_vs_fp32_oracle(hip_lib, t2v):
    """the pruned loop may not be further from the fp32 loop than 1.5 x the unpruned loop of the same model (tests/util.py)"""
    from open_sora_amd import sampling

    cfg, args, truth = _args(t2v)
    model = _build(cfg)
    den = sampling.I2VDenoiser()
    with torch.inference_mode():
        pruned = den.denoise(model, cfg_prune=True, **dict(args))
        unpruned = sampling.I2VDenoiser().denoise(model, **dict(args))
        torch.cuda.synchronize()
    full = 2 if t2v else 3
    assert den.last_branch_counts == [1 if i in (11, 13) else full for i in range(STEPS)]
    assert_parity(pruned, truth, unpruned, f"pruned {'t2v' if t2v else 'i2v'} loop, {STEPS} steps, vs fp32; comparator: the unpruned loop")


def test_pruned_loop_under_hipgraph_is_the_eager_pruned_loop(hip_lib, monkeypatch):
    """one graph per branch count in use: (3, 1) with an image condition, (2, 1) without -- a loop of cfg_branch_counts never holds
    more than two counts, so the three batch sizes are captured over the two runs, all on the one side stream of the device"""
    from open_sora_amd import sampling

    captured = []

    class Counting(torch.cuda.CUDAGraph):
        def capture_begin(self, *a, **k):
            captured.append(torch.cuda.current_stream().cuda_stream)
            return super().capture_begin(*a, **k)

    monkeypatch.setattr(torch.cuda, "CUDAGraph", Counting)
    model = None
    for t2v in (False, True):
        cfg, args, _ = _args(t2v)
        model = model or _build(cfg)
        with torch.inference_mode():
            eager = sampling.I2VDenoiser().denoise(model, cfg_prune=True, **dict(args))
            den = sampling.I2VDenoiser()
            graphed = den.denoise(model, cfg_prune=True, hip_graph=True, **dict(args))
            torch.cuda.synchronize()
        assert sorted(set(den.last_branch_counts)) == [1, 2 if t2v else 3]
        assert torch.isfinite(eager.float()).all()
        assert torch.equal(eager, graphed), f"{'t2v' if t2v else 'i2v'}: the replayed pruned loop differs from the eager one"
    side = sampling._SIDE_STREAMS[str(args["img"].device)].cuda_stream
    assert len(captured) == 4 and set(captured) == {side}, captured
