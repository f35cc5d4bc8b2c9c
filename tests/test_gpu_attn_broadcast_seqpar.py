"""GPU: attention broadcast under sequence parallelism -- the ranks-as-threads harness of tests/test_gpu_step_cache_seqpar.py on one
GPU, P = 2, both exchange modes, one store + reuse pair.  The store step is the sharded plain step bit for bit; the reuse step
exchanges nothing inside the blocks (one collective: the tail's gather); both steps of the pair, run on the same inputs, meet the
parity rule of tests/util.py against the fp32 oracle of that step, judged against the single-device pair's own error (a reuse step on
the inputs of its store step computes the store step); and the sharded reuse step on other inputs agrees with the single-device one
within the relative-L2 floor of that rule.  Each figure is printed before it is asserted (pytest -s)."""
import copy
import functools

import pytest
import torch

from oracle import configs, mmdit_oracle as O
from tests.local_transport import LocalTransport, run_ranks
from tests.test_gpu_mmdit import _build
from tests.test_gpu_row_kernels import bits
from tests.util import assert_parity, rel_l2, torch_inputs, torch_params

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF = torch.bfloat16
B_, T_, H_, W_, LT_ = 3, 2, 6, 6, 64                       # 64 text + 72 image tokens = 136 rows: 68 per rank
L_IMG = T_ * H_ * W_
ROWS = (0, 1, 2)


@functools.lru_cache(maxsize=None)
def _setup():
    """the tiny denoiser on the GPU with its plan built (shared and read-only once the rank threads start), its inputs, the fp32
    oracle of the step and the single-device pair; computed once, left unchanged"""
    cfg = dict(configs.GOLDEN["hd72_eager_split"][0], depth=2, depth_single_blocks=2)
    model = _build(cfg, DEV)
    a = torch_inputs(cfg, B_, T_, H_, W_, LT_, dtype=BF, device=DEV)
    b = dict(a, img=(a["img"].float() * 1.125).to(BF))
    with torch.inference_mode():
        truth = O.forward(torch_params(cfg), cfg, **torch_inputs(cfg, B_, T_, H_, W_, LT_))
        ac = model.attention_broadcast_begin(B_, LT_, L_IMG, DEV)
        store = model(**a, attn_cache=(ac, "store", ROWS)).clone()
        same = model(**a, attn_cache=(ac, "reuse", ROWS)).clone()
        other = model(**b, attn_cache=(ac, "reuse", ROWS)).clone()
    torch.cuda.synchronize()
    return cfg, model, a, b, truth, store.cpu(), same.cpu(), other.cpu()


@pytest.mark.parametrize("mode", ["allgather", "ulysses"])
def test_store_and_reuse_pair_on_two_ranks(hip_lib, mode):
    from open_sora_amd import seqpar

    cfg, model, a, b, truth, single_store, single_same, single_other = _setup()

    def rank_fn(rank, world):
        m = copy.copy(model)                       # shares parameters and plan; own sequence-parallel state, workspaces and cache
        m.forward = m.forward_ckpt
        object.__setattr__(m, "_osk_ws_cache", {})
        m.__dict__.pop("_osk_attn_cache", None)
        tp = LocalTransport(world, rank, DEV)
        sp = seqpar.enable(m, mode=mode, transport=tp)
        with torch.inference_mode():
            plain = m(**a).clone()
            n_plain = tp.calls
            ac = m.attention_broadcast_begin(B_, LT_, L_IMG, DEV)
            store = m(**a, attn_cache=(ac, "store", ROWS)).clone()
            n_store = tp.calls - n_plain
            same = m(**a, attn_cache=(ac, "reuse", ROWS)).clone()
            n_reuse = tp.calls - n_plain - n_store
            other = m(**b, attn_cache=(ac, "reuse", ROWS)).clone()
        torch.cuda.current_stream().synchronize()
        assert sp.geom == (68, 68) and ac.shard == (68 * rank, 68 * rank + 68) and tuple(ac.slots.shape) == (4, B_, 68, cfg["hidden_size"])
        return plain.cpu(), store.cpu(), same.cpu(), other.cpu(), (n_plain, n_store, n_reuse)

    res = run_ranks(2, rank_fn, DEV)
    for r in res[1:]:
        assert all(torch.equal(bits(x), bits(y)) for x, y in zip(r[:4], res[0][:4])), "ranks disagree"
    plain, store, same, other, (n_plain, n_store, n_reuse) = res[0]
    assert n_store == n_plain > 5 and n_reuse == 1, (n_plain, n_store, n_reuse)     # a reuse step: the tail's gather alone
    assert torch.equal(bits(store), bits(plain)), "a sharded store step is not the sharded plain step"
    what = f"attention broadcast under sequence parallelism, P = 2 {mode}"
    assert_parity(store, truth, single_store, f"{what}: store step vs the fp32 oracle; comparator: the single-device store step")
    assert_parity(same, truth, single_same, f"{what}: reuse step on the store step's inputs vs the fp32 oracle; comparator: single device")
    e = rel_l2(other, single_other)
    print(f"{what}: reuse step on other inputs, sharded vs single device: relL2 {e:.3e}; allowed 2^-8 = {2.0 ** -8:.3e}")
    assert e <= 2.0 ** -8
