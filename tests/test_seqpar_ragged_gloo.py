"""CPU, world_size 2 and 4 over gloo: sequence parallelism over joint lengths the rank count does NOT divide
(open_sora_amd/seqpar.py: ranks 0 .. P-2 own Lc = ceil(L / P) rows, the last one the rest; equal-sized collectives over
zero-padded slots; attention through osk_attention_fwd_ragged_bf16) must reproduce the single-process result and the oracle,
with the comparison and tolerances of tests/test_seqpar_gloo.py.  Kernels: the CPU emulation (tests/cpu_ops_ragged.py).
Plus the split rule itself, on the host."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, name, geom, q, mode, fp8):
    import torch.distributed as dist

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.set_num_threads(2)
        from open_sora_amd import mmdit, seqpar
        from oracle import configs
        from tests import cpu_ops_ragged
        from tests.util import torch_inputs, torch_params

        mmdit.set_ops_for_testing(cpu_ops_ragged)
        cfg = configs.GOLDEN[name][0]
        B, T, h, w, L_txt = geom
        model = mmdit.Flux(device_map="cpu", torch_dtype=torch.bfloat16, **cfg)
        model.load_state_dict(torch_params(cfg, dtype=torch.bfloat16), strict=True)
        if fp8:   # True: e4m3 V^T (pv8); "qk8": e4m3 K as well (head_dim 128)
            model.enable_fp8(qk8=fp8 == "qk8")
        inp = torch_inputs(cfg, B, T, h, w, L_txt, dtype=torch.bfloat16)
        with torch.inference_mode():
            single = model(**inp).float().clone()
            assert not cpu_ops_ragged.RAGGED_CALLS
            sp = seqpar.enable(model, mode=mode, kv_chunks=4)     # (a ragged split keeps the single gather whatever kv_chunks says)
            assert sp.head_parallel(cfg["num_heads"]) == (mode == "ulysses")
            sharded = model(**inp).float().clone()
            seqpar.disable(model)
        q.put((rank, single.numpy(), sharded.numpy(), list(cpu_ops_ragged.RAGGED_CALLS), sp.geom))
    except BaseException:  # surface the failure instead of letting the parent wait for the queue timeout
        import traceback

        q.put((rank, "error", traceback.format_exc()))
        raise
    finally:
        dist.destroy_process_group()


def _run(world, name, geom, mode, fp8=False):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, name, geom, q, mode, fp8)) for r in range(world)]
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
        p.join(timeout=60)
        assert p.exitcode == 0
    return sorted(res, key=lambda r: r[0])


# (world, golden config name, (B, T, h, w, L_txt)): L = L_txt + T*h*w with L % world in {1, world - 1}, ceil(L / world) > L_txt
CASES = [
    (2, "hd64_eager_fused", (2, 2, 2, 3, 5)),      # L = 17: 9 + 8
    (4, "hd72_eager_split", (2, 2, 3, 5, 3)),      # L = 33, L % 4 = 1: 9 + 9 + 9 + 6
    (4, "hd72_eager_split", (2, 2, 3, 5, 5)),      # L = 35, L % 4 = 3: 9 + 9 + 9 + 8
    (2, "hd128_liger_split", (3, 1, 2, 3, 3)),     # L = 9: 5 + 4, CFG-triple batch
    (2, "hd72_liger_fused", (1, 5, 3, 7, 24)),     # L = 129: 65 + 64 -- the last rank's chunk ends one 64-key tile earlier
]
IDS = lambda v: v if isinstance(v, str) else f"w{v[0]}-{v[1]}-L{v[2][4] + v[2][1] * v[2][2] * v[2][3]}"


def _check_split(res, world, L, mode, fp8):
    Lc = -(-L // world)
    for rank, _, _, calls, geom in res:
        assert geom == (Lc, L - (world - 1) * Lc)
        assert calls, "the ragged entry was not called"
        for kind, n_seg, seg_len, last in calls:
            want = fp8 if isinstance(fp8, str) else ("pv8" if fp8 else "bf16")
            assert (kind, n_seg, seg_len, last) == (want, world, Lc, L - (world - 1) * Lc), (kind, n_seg, seg_len, last)


@pytest.mark.parametrize("mode", ["allgather", "ulysses"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_ragged_seqpar_matches_single_process_and_oracle(case, mode):
    world, name, geom = case
    from oracle import configs, mmdit_oracle as O
    from tests.util import rel_l2, torch_inputs, torch_params

    cfg = configs.GOLDEN[name][0]
    B, T, h, w, L_txt = geom
    L = L_txt + T * h * w
    assert L % world in (1, world - 1) and -(-L // world) > L_txt
    res = _run(world, name, geom, mode)
    _check_split(res, world, L, mode, False)
    with torch.inference_mode():
        truth = O.forward(torch_params(cfg), cfg, **torch_inputs(cfg, B, T, h, w, L_txt))
        ref_bf16 = O.forward(torch_params(cfg, dtype=torch.bfloat16), cfg,
                             **torch_inputs(cfg, B, T, h, w, L_txt, dtype=torch.bfloat16))
    e_ref = rel_l2(ref_bf16.float(), truth)
    for rank, single, sharded, _, _ in res:
        single, sharded = torch.from_numpy(single), torch.from_numpy(sharded)
        assert sharded.shape == single.shape
        e1, eP = rel_l2(single, truth), rel_l2(sharded, truth)
        print(f"rank {rank}: relL2 single {e1:.3e} sharded {eP:.3e} ref-bf16 {e_ref:.3e}")
        assert eP <= max(1.5 * e_ref, 2.0 ** -8), (rank, eP, e_ref)
        assert rel_l2(sharded, single) <= 2.0 ** -7, (rank, rel_l2(sharded, single))
    for rank, _, sharded, _, _ in res[1:]:  # every rank returns the same full prediction
        assert np.array_equal(sharded, res[0][2])


@pytest.mark.parametrize("case,mode", [(CASES[3], "allgather"), (CASES[4], "allgather"), (CASES[1], "ulysses"), (CASES[4], "ulysses")],
                         ids=IDS)
def test_ragged_seqpar_fp8_mode(case, mode):
    """the fp8 handles (e4m3 V^T, scale agreed across the ranks) on a ragged split: sharded == single-process fp8 mode within the
    bound tests/test_seqpar_gloo.py::test_seqpar_fp8_mode applies"""
    world, name, geom = case
    from tests.util import rel_l2

    res = _run(world, name, geom, mode, fp8=True)
    _check_split(res, world, geom[4] + geom[1] * geom[2] * geom[3], mode, True)
    for rank, single, sharded, _, _ in res:
        single, sharded = torch.from_numpy(single), torch.from_numpy(sharded)
        assert rel_l2(sharded, single) <= 2e-2, (rank, rel_l2(sharded, single))
    for rank, _, sharded, _, _ in res[1:]:
        assert np.array_equal(sharded, res[0][2])


@pytest.mark.parametrize("mode", ["allgather", "ulysses"])
def test_ragged_seqpar_qk8_mode(mode):
    """enable_fp8(qk8=True) at head_dim 128 on a ragged split: K travels (all-gather) or is packed after the exchange (head exchange) as
    e4m3 with the last rank's chunk packed as a tensor of its own rows; every rank's attention is the ragged entry on qk8 operands.
    Bound: the one tests/test_seqpar_qk8_host.py applies between the sharded and the single-process forward."""
    world, name, geom = CASES[3]
    from tests.util import rel_l2

    res = _run(world, name, geom, mode, fp8="qk8")
    _check_split(res, world, geom[4] + geom[1] * geom[2] * geom[3], mode, "qk8")
    for rank, single, sharded, _, _ in res:
        single, sharded = torch.from_numpy(single), torch.from_numpy(sharded)
        assert rel_l2(sharded, single) <= 2e-2, (rank, rel_l2(sharded, single))
    for rank, _, sharded, _, _ in res[1:]:
        assert np.array_equal(sharded, res[0][2])


class _Tp:
    def __init__(self, P, rank):
        self.P, self.rank = P, rank


def test_split_rule_tiles_the_sequence():
    """for every L <= 4096 and P <= 8: the ranks' ranges tile [0, L) in order, every rank owns >= 1 row or shard_range is None on every
    rank, the first P - 1 ranks own ceil(L / P) rows, and P | L reproduces the equal split [r L/P, (r + 1) L/P)"""
    from open_sora_amd import seqpar

    for P in range(1, 9):
        sps = [seqpar.SeqPar(transport=_Tp(P, r), mode="allgather") for r in range(P)]
        for L in range(1, 4097):
            for L_txt in (0, L // 3):
                rs = [sp.shard_range(L, L_txt) for sp in sps]
                Lc = -(-L // P)
                if P == 1 or L - (P - 1) * Lc < 1 or Lc <= L_txt:
                    assert rs == [None] * P, (P, L, L_txt, rs)
                    continue
                assert rs[0][0] == 0 and rs[-1][1] == L and all(a[1] == b[0] for a, b in zip(rs, rs[1:])), (P, L, rs)
                assert all(hi - lo == Lc for lo, hi in rs[:-1]) and 1 <= rs[-1][1] - rs[-1][0] <= Lc, (P, L, rs)
                assert all(sp.geom == (Lc, rs[-1][1] - rs[-1][0]) for sp in sps)
                if L % P == 0:
                    assert rs == [(r * (L // P), (r + 1) * (L // P)) for r in range(P)], (P, L, rs)


def test_ragged_split_reporting():
    """a ragged split keeps the single gather, and says so"""
    from open_sora_amd import seqpar

    sp = seqpar.SeqPar(transport=_Tp(4, 1), mode="allgather", kv_chunks=4)
    assert sp.shard_range(4 * 80, 16) == (80, 160) and sp.kv_chunks_for(80) == 4
    assert sp.shard_range(4 * 80 + 1, 16) == (81, 162) and sp.geom == (81, 78)
    assert sp.kv_chunks_for(81) == 1 and sp.kv_chunks_applied(8, False, 81, 78) == 1 and sp.kv_chunks_applied(8, False, 80, 80) == 4
