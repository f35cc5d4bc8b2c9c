"""GPU: the fp8 QK^T attention (qk8) under sequence parallelism.

  * osk_kv_scale_fp8 against two osk_v_scale_fp8 calls, bit for bit, on strided views, with guard bands round the output;
  * the property that makes the sequence-parallel result the single-device quantisation: P segments of K packed separately with
    the max-reduced scales are, concatenated, the bytes osk_k_pack_fp8 makes of the whole K;
  * one device, two processes, the collectives staged through the host exactly as in tests/test_gpu_seqpar_1gpu.py (its helpers
    are imported, not copied): with enable_fp8(qk8=True) every rank runs osk_attention_fwd_qk8_bf16 once per block and never the
    pv8 entry, in both exchange modes, whole and ragged segments; the output is held against the single-process qk8 forward
    (that file's fp8 bound) and against the fp32 oracle (the project's fp8 gate);
  * head_dim 72 and qk8=False keep the pv8 exchange.
The measured errors are recorded in profiles/attn_qk8_sp.md."""
import os

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from tests.test_gpu_kernels import BF, DEV, rnd
from tests.test_gpu_seqpar_1gpu import _free_port, _stage_collectives_through_host

pytestmark = pytest.mark.gpu

SENTINEL = -12345.0


# ----------------------------------------------------------------------------------------------- osk_kv_scale_fp8
# L = 130: the issue's ragged case (one round of the block, most of its row indices clamped to the last row).  The longer ones
# take several rounds of 8 passes of 1024 / (hd / 8) rows: 512 rows at head_dim 128 (1100 = two whole rounds + a clamped one),
# 904 at head_dim 72 (2000 likewise).
@pytest.mark.parametrize("hd,L", [(128, 130), (72, 130), (128, 1100), (72, 2000)])
def test_kv_scale_fp8_equals_two_v_scale_calls(hip_lib, hd, L):
    B, H = 2, 3
    D = H * hd
    y = rnd("y", (B, L, 3 * D), std=1.1, seed=301)          # one fused [q | k | v] buffer: row stride 3 D, not D
    k, v = y[:, :, D: 2 * D], y[:, :, 2 * D:]
    k[1, :, hd: 2 * hd] = 0                                   # all-zero heads: scale 1.0
    v[0, :, 2 * hd:] = 0
    k[0, L - 1, D - 1] = 300.0                                # outliers in the last row / last column and the first of each
    v[1, 0, 0] = -250.0
    assert k.stride(1) == 3 * D and not k.is_contiguous()
    G = 64
    big = torch.full((2 * B * H + 2 * G,), SENTINEL, dtype=torch.float32, device=DEV)
    out = big[G: G + 2 * B * H].view(2, B, H)
    s = hip_lib.kv_scale_fp8(k, v, H, hd, out=out)
    assert s.data_ptr() == out.data_ptr()
    sk, sv = hip_lib.v_scale_fp8(k, H, hd), hip_lib.v_scale_fp8(v, H, hd)
    assert torch.equal(s[0], sk) and torch.equal(s[1], sv)
    assert s[0, 1, 1] == 1.0 and s[1, 0, 2] == 1.0
    assert s[0, 0, H - 1].item() == (torch.tensor(300.0) / 448.0).item() and s[1, 1, 0].item() == (torch.tensor(250.0) / 448.0).item()
    assert bool((big[:G] == SENTINEL).all()) and bool((big[G + 2 * B * H:] == SENTINEL).all())
    fresh = hip_lib.kv_scale_fp8(k, v, H, hd)                # the allocating form
    assert fresh.shape == (2, B, H) and torch.equal(fresh, s)


# ----------------------------------------------------------------------------------------------- gathered K bytes
def test_segments_packed_with_reduced_scales_are_the_single_device_bytes(hip_lib):
    P, B, H, Lloc, hd = 2, 2, 3, 128, 128
    D = H * hd
    y = rnd("y", (B, P * Lloc, 3 * D), std=1.2, seed=311)
    k, v = y[:, :, D: 2 * D], y[:, :, 2 * D:]
    k[0, 5, 7] = 77.0                                         # rank 0 owns head (0, 0)'s scale, rank 1 head (1, 2)'s
    k[1, Lloc + 9, D - 3] = -91.0
    whole = hip_lib.kv_scale_fp8(k, v, H, hd)
    k8_whole = torch.empty(hip_lib.k8_shape(B, H, P * Lloc), dtype=torch.uint8, device=DEV)
    hip_lib.k_pack_fp8(k, whole[0], k8_whole, H, hd)
    parts = [hip_lib.kv_scale_fp8(k[:, r * Lloc: (r + 1) * Lloc], v[:, r * Lloc: (r + 1) * Lloc], H, hd) for r in range(P)]
    reduced = torch.stack(parts).amax(0).contiguous()         # what all_reduce_max leaves on every rank
    assert torch.equal(reduced, whole) and not torch.equal(parts[0], parts[1])
    k8_all = torch.full((P, *hip_lib.k8_shape(B, H, Lloc)), 0xAA, dtype=torch.uint8, device=DEV)
    for r in range(P):
        hip_lib.k_pack_fp8(k[:, r * Lloc: (r + 1) * Lloc], reduced[0], k8_all[r], H, hd)
    assert torch.equal(torch.cat(list(k8_all), 2), k8_whole)


# ----------------------------------------------------------------------------------------------- two processes, one device
def _worker(rank, world, port, name, over, geom, q, mode, qk8):
    import torch.distributed as dist

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.cuda.set_device(0)
        torch.set_num_threads(4)
        _stage_collectives_through_host(dist)
        from open_sora_amd import mmdit, seqpar
        from oracle import configs
        from tests.util import torch_inputs, torch_params

        ops = mmdit.ops()
        n = {"qk8": 0, "pv8": 0, "reduce": 0}
        real_qk8, real_pv8, real_ar = ops.attention_fwd_qk8, ops.attention_fwd_pv8, dist.all_reduce
        ops.attention_fwd_qk8 = lambda *a, **k: (n.__setitem__("qk8", n["qk8"] + 1), real_qk8(*a, **k))[1]
        ops.attention_fwd_pv8 = lambda *a, **k: (n.__setitem__("pv8", n["pv8"] + 1), real_pv8(*a, **k))[1]
        dist.all_reduce = lambda *a, **k: (n.__setitem__("reduce", n["reduce"] + 1), real_ar(*a, **k))[1]
        cfg = dict(configs.GOLDEN[name][0], **over)
        model = mmdit.Flux(device_map="cuda:0", torch_dtype=torch.bfloat16, **cfg)
        model.load_state_dict(torch_params(cfg, dtype=torch.bfloat16, device="cuda:0"), strict=True)
        model.enable_fp8(qk8=qk8)
        inp = torch_inputs(cfg, *geom, dtype=torch.bfloat16, device="cuda:0")
        with torch.inference_mode():
            single = model(**inp).float().cpu()
            n_single = dict(n)
            n.update(qk8=0, pv8=0, reduce=0)
            sp = seqpar.enable(model, mode=mode)
            assert model._sp is not None and sp.P == world
            outs = [model(**inp).float().cpu() for _ in range(2)]
            n_sp = dict(n)
            other = None
            if qk8:       # the same sharded step with the flag off: what the flag must not change where the kernel does not apply
                other = model.enable_fp8(qk8=False)(**inp).float().cpu().numpy()
            seqpar.disable(model)
        assert torch.equal(outs[0], outs[1]), "the sequence-parallel forward is not repeatable"
        q.put((rank, single.numpy(), outs[0].numpy(), n_single, n_sp, other))
    except BaseException:
        import traceback

        q.put((rank, "error", traceback.format_exc()))
        raise
    finally:
        dist.destroy_process_group()


def _run(world, name, over, geom, mode, qk8):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, name, over, geom, q, mode, qk8)) for r in range(world)]
    for p in procs:
        p.start()
    res = []
    for _ in range(world):
        r = q.get(timeout=600)
        if isinstance(r[1], str):
            for p in procs:
                p.kill()
            pytest.fail(f"rank {r[0]} failed:\n{r[2]}")
        res.append(r)
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    return sorted(res, key=lambda r: r[0])


SMALL = dict(depth=1, depth_single_blocks=1)          # the small head_dim-128 model of tests/test_gpu_fp8.py::test_mmdit_forward_fp8_mode
GEOMS = {"whole": (2, 2, 12, 16, 128),                # L = 512: 256 keys per rank, whole 64-key tiles
         "ragged": (2, 2, 12, 12, 160)}               # L = 448: 224 keys per rank, 224 % 64 = 32 (that test's geometry)
_TRUTH = {}


def _truth(cfg, geom):
    """fp32 oracle of one geometry, computed once and shared by the two exchange modes"""
    from oracle import mmdit_oracle as O
    from tests.util import torch_inputs, torch_params

    if geom not in _TRUTH:
        with torch.inference_mode():
            _TRUTH[geom] = O.forward(torch_params(cfg), cfg, **torch_inputs(cfg, *geom))
    return _TRUTH[geom]


@pytest.mark.parametrize("mode", ["allgather", "ulysses"])
@pytest.mark.parametrize("geom", list(GEOMS), ids=list(GEOMS))
def test_qk8_forward_under_sequence_parallelism_two_processes_one_gpu(hip_lib, geom, mode):
    from oracle import configs
    from tests.util import rel_l2

    P, g = 2, GEOMS[geom]
    cfg = dict(configs.GOLDEN["hd128_eager_fused"][0], **SMALL)
    n_blocks = cfg["depth"] + cfg["depth_single_blocks"]
    L = g[4] + g[1] * g[2] * g[3]
    assert L % P == 0 and L // P > g[4] and ((L // P) % 64 == 0) == (geom == "whole")
    res = _run(P, "hd128_eager_fused", SMALL, g, mode, True)
    truth = _truth(cfg, g)
    for rank, single, sharded, n_single, n_sp, _ in res:
        single, sharded = torch.from_numpy(single), torch.from_numpy(sharded)
        e_s, e_t, e_1 = rel_l2(sharded, single), rel_l2(sharded, truth), rel_l2(single, truth)
        print(f"{geom} {mode} rank {rank}: relL2 SP vs single {e_s:.3e}, SP vs fp32 {e_t:.3e}, single vs fp32 {e_1:.3e}; calls {n_sp}")
        assert (n_single["qk8"], n_single["pv8"]) == (n_blocks, 0)
        assert (n_sp["qk8"], n_sp["pv8"]) == (2 * n_blocks, 0), n_sp                     # two forwards
        assert n_sp["reduce"] == (2 * n_blocks if mode == "allgather" else 0), n_sp      # ONE reducing collective per block, or none
        assert e_s <= 2e-2, (rank, e_s)                                                  # tests/test_gpu_seqpar_1gpu.py, fp8 case
        assert e_t <= 5e-2, (rank, e_t)                                                  # the project's fp8 gate
    assert np.array_equal(res[1][2], res[0][2]), "ranks disagree on the gathered prediction"


@pytest.mark.parametrize("mode", ["allgather", "ulysses"])
def test_head_dim_72_keeps_the_pv8_exchange(hip_lib, mode):
    from tests.util import rel_l2

    res = _run(2, "hd72_eager_split", {}, (2, 4, 8, 8, 64), mode, True)
    for rank, single, sharded, n_single, n_sp, flag_off in res:
        assert (n_single["qk8"], n_single["pv8"]) == (0, 3)
        assert (n_sp["qk8"], n_sp["pv8"]) == (0, 2 * 3), n_sp                            # two forwards of three blocks
        assert n_sp["reduce"] == (2 * 3 if mode == "allgather" else 0)
        assert np.array_equal(sharded, flag_off)                                          # exactly what enable_fp8() computes
        assert rel_l2(torch.from_numpy(sharded), torch.from_numpy(single)) <= 2e-2
    assert np.array_equal(res[1][2], res[0][2])


@pytest.mark.parametrize("mode", ["allgather", "ulysses"])
def test_without_the_flag_head_dim_128_keeps_the_pv8_exchange(hip_lib, mode):
    from tests.util import rel_l2

    res = _run(2, "hd128_eager_fused", SMALL, GEOMS["ragged"], mode, False)
    for rank, single, sharded, n_single, n_sp, _ in res:
        assert (n_single["qk8"], n_single["pv8"]) == (0, 2)
        assert (n_sp["qk8"], n_sp["pv8"]) == (0, 2 * 2), n_sp
        assert n_sp["reduce"] == (2 * 2 if mode == "allgather" else 0)
        e_s = rel_l2(torch.from_numpy(sharded), torch.from_numpy(single))
        print(f"pv8 (no flag), ragged {mode} rank {rank}: relL2 SP vs single {e_s:.3e}")
        assert e_s <= 2e-2, (rank, e_s)
    assert np.array_equal(res[1][2], res[0][2])
