"""CPU: the host side of the sampler's attention broadcast (I2VDenoiser.denoise(attn_broadcast=...), open_sora_amd/sampling.py;
MMDiTModel.forward_ckpt(attn_cache=...), open_sora_amd/mmdit.py): the schedule as a pure function, the launch trace of a plain, a
store and a reuse forward on the CPU kernel table (tests/cpu_ops_attn_broadcast.py), the reuse semantics bit for bit, the loop against
a loop driven by hand, the refusals and the binding.  The kernel and the GPU loop: tests/test_gpu_attn_broadcast.py."""
import os

import pytest
import torch

from oracle import configs
from tests import cpu_ops_attn_broadcast as AB
from tests.test_step_cache_host import _bf, _case
from tests.util import torch_inputs, torch_params

BF = torch.bfloat16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ----------------------------------------------------------------------------- the schedule
def _plan(n, interval, t_range=(0.0, 1.0)):
    from open_sora_amd.sampling import attn_broadcast_plan

    ts = [1.0 - i / max(n, 1) for i in range(n + 1)]      # step i runs at t = 1 - i / n
    return attn_broadcast_plan(ts, interval, t_range)


def test_first_and_last_step_are_plain():
    for interval in (2, 3, 5):
        p = _plan(10, interval)
        assert len(p) == 10 and p[0] == "plain" and p[-1] == "plain"
    assert _plan(1, 2) == ["plain"] and _plan(2, 2) == ["plain", "plain"] and _plan(0, 2) == []
    assert _plan(3, 2) == ["plain", "plain", "plain"]      # one inner step: computed, nothing behind it to reuse


def test_range_edges_are_inclusive():
    # n = 8: t = 1, .875, .75, .625, .5, .375, .25, .125 -- all exact in binary
    assert _plan(8, 2, (0.25, 0.75)) == ["plain", "plain", "store", "reuse", "store", "reuse", "plain", "plain"]
    assert _plan(8, 2, (0.2500001, 0.75)) == ["plain", "plain", "store", "reuse", "store", "reuse", "plain", "plain"]
    assert _plan(8, 2, (0.25, 0.7499999)) == ["plain", "plain", "plain", "store", "reuse", "store", "reuse", "plain"]
    assert _plan(8, 2, (0.375, 0.625)) == ["plain", "plain", "plain", "store", "reuse", "plain", "plain", "plain"]
    assert _plan(8, 2, (0.5, 0.5)) == ["plain"] * 8        # one step inside: computed, plain
    assert _plan(8, 2, (2.0, 3.0)) == ["plain"] * 8


def test_intervals():
    assert _plan(8, 1) == ["plain"] * 8 and _plan(8, 0) == ["plain"] * 8 and _plan(8, -3) == ["plain"] * 8
    assert _plan(8, 2) == ["plain", "store", "reuse", "store", "reuse", "store", "reuse", "plain"]
    assert _plan(8, 3) == ["plain", "store", "reuse", "reuse", "store", "reuse", "reuse", "plain"]
    assert _plan(8, 4) == ["plain", "store", "reuse", "reuse", "reuse", "store", "reuse", "plain"]
    assert _plan(8, 100) == ["plain", "store"] + ["reuse"] * 5 + ["plain"]          # larger than the range: one cycle


@pytest.mark.parametrize("n", [2, 5, 9, 30, 50])
@pytest.mark.parametrize("interval", [2, 3, 4, 7])
def test_store_only_before_a_reuse_and_every_cycle_has_a_computed_step(n, interval):
    from open_sora_amd.sampling import ATTN_BROADCAST_RANGE, attn_broadcast_plan, get_schedule

    for ts, rng in (([1.0 - i / n for i in range(n + 1)], (0.0, 1.0)), (get_schedule(n, 1024, 17), ATTN_BROADCAST_RANGE)):
        p = attn_broadcast_plan(ts, interval, rng)
        assert len(p) == n and set(p) <= {"plain", "store", "reuse"}
        run = 0
        for i, m in enumerate(p):
            if m == "store":
                assert p[i + 1] == "reuse"
            if m == "reuse":
                run += 1
                assert p[i - 1] in ("store", "reuse") and rng[0] <= ts[i] <= rng[1] and 0 < i < n - 1
                assert run <= interval - 1                # never two cycles without a computed step between them
            else:
                run = 0
            if m == "plain" and i + 1 < n:
                assert p[i + 1] != "reuse"
        # a pure function of its arguments
        assert attn_broadcast_plan(list(ts), interval, tuple(rng)) == p


def test_effective_modes_follow_the_rows():
    from open_sora_amd.sampling import attn_broadcast_effective

    plan = ["plain", "store", "reuse", "reuse", "store", "reuse", "reuse", "plain"]
    assert attn_broadcast_effective(plan, [3] * 8) == plan
    # a one-branch store, then a three-branch reuse: rows 1 and 2 hold nothing -> computed and stored; the next reuses
    assert attn_broadcast_effective(plan, [3, 1, 3, 1, 3, 1, 3, 3]) == ["plain", "store", "store", "reuse", "store", "reuse", "reuse", "plain"]
    assert attn_broadcast_effective(plan, [1, 1, 1, 3, 1, 1, 3, 3], n=2) == ["plain", "store", "reuse", "store", "store", "reuse", "store", "plain"]


# ----------------------------------------------------------------------------- the model on the CPU kernel table
B_, T_, H_, W_, LT_ = 3, 2, 4, 6, 8               # 2 frames x 2 x 3 = 12 ... torch_inputs: h, w in patches -> 48 image tokens


@pytest.fixture()
def ab_ops(hip_lib, monkeypatch):
    from open_sora_amd import mmdit

    for k in ("OSK_ATTN_BROADCAST", "OSK_STEP_CACHE", "OSK_CFG_PRUNE", "OSK_ATTN_WINDOW_FRAMES", "OSK_SP_KV_CHUNKS", "OSK_SP_MODE"):
        monkeypatch.delenv(k, raising=False)
    mmdit.set_ops_for_testing(AB)
    AB.AB_CALLS.clear()
    yield mmdit
    mmdit.set_ops_for_testing(hip_lib)


def _tiny(mmdit, **over):
    cfg = dict(configs.GOLDEN["hd72_eager_split"][0], depth=2, depth_single_blocks=2, **over)
    model = mmdit.Flux(device_map="cpu", torch_dtype=BF, **cfg)
    model.load_state_dict(torch_params(cfg, dtype=BF), strict=True)
    return cfg, model


def _shift(inp, s):
    return dict(inp, img=(inp["img"].float() * (1.0 + s)).to(BF), timesteps=(inp["timesteps"].float() * (1.0 - s)).to(BF))


# The launches of one forward of the tiny model (depth 2 + 2, B 3, 8 text + 48 image tokens, hidden 576, 8 heads of 72) as the PARENT
# commit makes them: (entry, shapes of the tensor arguments), recorded there with tests/cpu_ops_attn_broadcast.py::Traced.
_D, _LI, _L = 576, 48, 56
_MOD = ((B_, _D), (B_, _D))


def _pair(k_in, n_out, gated):
    side = lambda l: (("a", (B_, l, k_in)), ("bias", (n_out,))) + ((("gate", (B_, _D)),) if gated else ()) + (("out", (B_, l, n_out)),) + \
        ((("res", (B_, l, n_out)),) if gated else ()) + (("w", (n_out, k_in)),)
    return ("gemm_pair", (side(_LI), side(LT_)))


_LN2 = [("ln_modulate", ((B_, _LI, _D),) + _MOD + ((B_, _LI, _D),)), ("ln_modulate", ((B_, LT_, _D),) + _MOD + ((B_, LT_, _D),))]
_ATTN = [("qknorm_rope", ((B_, _L, _D), (B_, _L, _D), (72,), (72,), (72,), (72,), (B_, _L, 36), (B_, _L, 36))),
         ("v_transpose", ((B_, _L, _D), (B_, 8, 72, 64))),
         ("attention_fwd", ((B_, _L, _D), (B_, _L, _D), (B_, 8, 72, 64), (B_, _L, _D), ("workspace", (16,))))]
_HEAD = [("copy_rows", ((B_, _LI, 64), (B_, _LI, 192))), ("copy_rows", ((B_, _LI, 68), (B_, _LI, 128))),
         ("gemm", ((B_, _LI, 192), (_D, 192), (_D,), (B_, _LI, _D))), ("gemm", ((B_, LT_, 128), (_D, 128), (_D,), (B_, LT_, _D))),
         ("timestep_embedding", ((B_,), (B_, 256))), ("gemv_tasks", ((B_, 256), (B_, _D))), ("gemv_tasks", ((B_, _D), (B_, _D))),
         ("gemv_tasks", ((B_, 48), (B_, _D))), ("gemv_tasks", ((B_, _D), (B_, _D))), ("rope_table", ((B_ * _L, 3), (B_, _L, 36), (B_, _L, 36))),
         ("gemv_tasks", ((B_, _D), (B_, 18432)))]
_DOUBLE_REST = [_pair(_D, _D, True)] + _LN2 + [_pair(_D, 4 * _D, False), _pair(4 * _D, _D, True)]
_DOUBLE = _LN2 + [_pair(_D, 3 * _D, False)] + _ATTN + _DOUBLE_REST
_SINGLE_LN = ("ln_modulate", ((B_, _L, _D),) + _MOD + ((B_, _L, _D),))
_SINGLE_L2 = ("gemm", ((B_, _L, 5 * _D), (_D, 5 * _D), (_D,), (B_, _L, _D), ("gate", (B_, _D)), ("res", (B_, _L, _D))))
_SINGLE = [_SINGLE_LN, ("gemm", ((B_, _L, _D), (7 * _D, _D), (7 * _D,), (B_, _L, 7 * _D)))] + _ATTN + [_SINGLE_L2]
_TAIL = [("ln_modulate", ((B_, _LI, _D),) + _MOD + ((B_, _LI, _D),)), ("gemm", ((B_, _LI, _D), (64, _D), (64,), (B_, _LI, 64)))]
PARENT_TRACE = _HEAD + _DOUBLE * 2 + _SINGLE * 2 + _TAIL
_COPY = ("attn_cache_copy", ((B_, _L, _D), (B_, _L, _D)))
_SINGLE_REUSE = [_SINGLE_LN, ("gemm", ((B_, _L, _D), (4 * _D, _D), (4 * _D,), (B_, _L, 4 * _D))), _COPY, _SINGLE_L2]
SKIPPED = ("attention_fwd", "qknorm_rope", "v_transpose", "k_pack_fp8", "rownorm2_max", "gemm_group")


def _traced_forwards(mmdit):
    """-> the traces of a plain, a store and a reuse forward of the tiny model (its plans built by a forward before)"""
    cfg, model = _tiny(mmdit)
    inp = torch_inputs(cfg, B_, T_, H_, W_, LT_, dtype=BF)
    log = []
    with torch.inference_mode():
        model(**inp)
        mmdit.set_ops_for_testing(AB.Traced(AB, log))
        model(**inp)                                    # (another kernel table: this forward builds its own workspaces)
        out = []
        ac = model.attention_broadcast_begin(B_, LT_, _LI, "cpu")
        for extra in ({}, {"attn_cache": (ac, "store", (0, 1, 2))}, {"attn_cache": (ac, "reuse", (0, 1, 2))}):
            del log[:]
            model(**inp, **extra)
            out.append(list(log))
    return out


def test_launch_traces(ab_ops):
    plain, store, reuse = _traced_forwards(ab_ops)
    assert len(PARENT_TRACE) == 47
    assert plain == PARENT_TRACE                         # attn_cache=None: the parent's forward, launch for launch
    # store: the same launches plus one copy behind every block's attention
    assert [e for e in store if e[0] != "attn_cache_copy"] == PARENT_TRACE
    copies = [i for i, e in enumerate(store) if e[0] == "attn_cache_copy"]
    assert len(copies) == 4 and all(store[i] == _COPY and store[i - 1][0] == "attention_fwd" for i in copies)
    # reuse: nothing of the attention path, the projections and MLPs as ever
    assert not [e for e in reuse if any(e[0].startswith(s) for s in SKIPPED)]
    assert reuse == _HEAD + _DOUBLE_REST * 2 + _SINGLE_REUSE * 2 + _TAIL
    gemms = lambda t: sum(2 if e[0] == "gemm_pair" else 1 for e in t if e[0] in ("gemm", "gemm_pair"))
    assert gemms(_SINGLE_REUSE) == 2 and gemms(_DOUBLE_REST) == 6             # per double block: 2 proj + 4 MLP GEMMs
    assert gemms(reuse) == gemms(_HEAD) + 2 * 6 + 2 * 2 + gemms(_TAIL)


def _forward_with_attention(monkeypatch, model, inp, per_block):
    """a plain forward in which the attention call of block j writes per_block[j] instead of computing"""
    calls = []

    def attention(q, k, vt, out, *args, **kw):
        out.copy_(per_block[len(calls)])
        calls.append(tuple(out.shape))

    with monkeypatch.context() as mp:
        mp.setattr(AB, "attention_fwd", attention)
        got = model(**inp).clone()
    assert len(calls) == len(per_block)
    return got


def test_reuse_equals_a_forward_whose_attention_returns_the_stored_tensor(ab_ops, monkeypatch):
    """store on inputs A leaves A's attention outputs in the slots; reuse on inputs B must equal, bit for bit, a plain forward on B in
    which every attention call writes the stored tensor of its block instead of computing"""
    cfg, model = _tiny(ab_ops)
    a = torch_inputs(cfg, B_, T_, H_, W_, LT_, dtype=BF)
    b = _shift(a, 0.125)
    with torch.inference_mode():
        plain_a = model(**a).clone()
        ac = model.attention_broadcast_begin(B_, LT_, _LI, "cpu")
        assert tuple(ac.slots.shape) == (4, B_, _L, _D) and ac.have == [False] * B_
        assert torch.equal(model(**a, attn_cache=(ac, "store", (0, 1, 2))), plain_a) and ac.have == [True] * B_
        assert torch.equal(model(**a, attn_cache=(ac, "reuse", (0, 1, 2))), plain_a)      # same inputs: the same attention output
        stored = ac.slots.clone()
        got = model(**b, attn_cache=(ac, "reuse", (0, 1, 2))).clone()
        assert torch.equal(ac.slots, stored)                                               # reuse reads only
        want = _forward_with_attention(monkeypatch, model, b, list(stored))
        plain_b = model(**b).clone()
    assert torch.equal(got, want)
    assert not torch.equal(got, plain_b) and not torch.equal(got, plain_a)


def test_rows_that_are_not_the_leading_ones_go_through_the_map(ab_ops, monkeypatch):
    cfg, model = _tiny(ab_ops)
    a = torch_inputs(cfg, B_, T_, H_, W_, LT_, dtype=BF)
    pick = lambda rows: {k: (v[list(rows)] if torch.is_tensor(v) and v.shape[0] == B_ else v) for k, v in a.items()}
    with torch.inference_mode():
        ac = model.attention_broadcast_begin(B_, LT_, _LI, "cpu")
        model(**a, attn_cache=(ac, "store", (0, 1, 2)))
        full = ac.slots.clone()
        for rows in ((2, 0), (0, 1), (1,), (0, 2)):      # (2, 0): no even spacing, the double blocks load through the map too
            got = model(**pick(rows), attn_cache=(ac, "reuse", rows)).clone()
            assert torch.equal(got, _forward_with_attention(monkeypatch, model, pick(rows), [s[list(rows)] for s in full])), rows
        assert torch.equal(ac.slots, full)
        ac.clear()
        ac.slots.zero_()
        model(**pick((2, 0)), attn_cache=(ac, "store", (2, 0)))
        assert ac.have == [True, False, True] and not ac.slots[:, 1].any() and ac.slots[:, 0].any() and ac.slots[:, 2].any()
        again = model(**pick((2, 0)), attn_cache=(ac, "reuse", (2, 0))).clone()
        assert torch.equal(again, _forward_with_attention(monkeypatch, model, pick((2, 0)), [s[[2, 0]] for s in ac.slots]))
    maps = [c[2] for c in AB.AB_CALLS[next(iter(AB.AB_CALLS))]]
    assert (2, 0) in maps and (1,) in maps and (0, 2) in maps and None in maps


# ----------------------------------------------------------------------------- the loop
def _hand_loop(model, tensors, kw, modes, counts=None, dev="cpu", ops=AB):
    """I2VDenoiser's loop driven by hand from forward_ckpt with the given mode per step (rows = the leading rows of the triple)"""
    from open_sora_amd import sampling

    t = {k: v.to(dev) for k, v in _bf(tensors).items()}
    ts = kw["timesteps"]
    n = t["img"].shape[0] // 3
    pruned = counts is not None
    counts = counts or [3] * (len(ts) - 1)
    cond = sampling.pack(torch.cat((t["masks"], t["masked_ref"]), dim=1))
    cond3 = torch.cat([cond, cond, torch.zeros_like(cond)], 0)
    x = t["img"][:n].clone()
    ac = model.attention_broadcast_begin(3 * n, t["txt"].shape[1], t["img"].shape[1], dev)
    for i, (t_curr, t_prev) in enumerate(zip(ts[:-1], ts[1:])):
        nb, mode = counts[i], modes[i]
        m = nb * n
        if mode != "reuse":
            ac.clear()
        extra = {} if mode == "plain" else {"attn_cache": (ac, mode, tuple(range(m)))}
        pred = model(img=x.repeat(nb, 1, 1), img_ids=t["img_ids"][:m], txt=t["txt"][:m], txt_ids=t["txt_ids"][:m], y_vec=t["y_vec"][:m],
                     cond=cond3[:m], timesteps=torch.full((m,), t_curr, dtype=BF, device=dev),
                     guidance=torch.full((m,), kw["guidance"], dtype=BF, device=dev), **extra)
        tg = sampling.get_oscillation_gs(kw["guidance"], i)
        ig = sampling.get_oscillation_gs(kw["guidance_img"], i)
        gvec = None
        if nb == 3 and ig > 1.0:
            b, c, tt, w_, h_ = t["masked_ref"].shape
            upper = torch.linspace(ig, 1.0, len(ts))[i]
            ramp = torch.linspace(1.0, float(upper), tt)[None, None, :, None, None].repeat(b, c, 1, h_, w_)
            gvec, ig = sampling.pack(ramp).to(dev, torch.float32).contiguous(), 1.0
        x_next = torch.empty_like(x)
        if pruned:
            ops.cfg_euler_nb(pred.contiguous(), nb, x, x_next, float(tg), float(ig), float(t_prev - t_curr), gvec)
        else:
            ops.cfg_euler(pred.contiguous(), x, x_next, float(tg), float(ig), float(t_prev - t_curr), gvec)
        x = x_next
    return x


def test_loop_equals_the_loop_driven_by_hand(ab_ops):
    from open_sora_amd import sampling
    from tests.test_step_cache_host import _model

    cfg, tensors, kw = _case()                            # 8 steps
    model = _model(ab_ops, cfg)
    ts = kw["timesteps"]
    rng = (ts[6], ts[2])                                  # covers steps 2 .. 6
    want_modes = ["plain", "plain", "store", "reuse", "store", "reuse", "plain", "plain"]
    assert sampling.attn_broadcast_plan(ts, 2, rng) == want_modes
    with torch.inference_mode():
        den = sampling.I2VDenoiser()
        out = den.denoise(model, attn_broadcast=2, attn_broadcast_range=rng, **_bf(tensors), **kw)
        assert den.last_attn_broadcast == want_modes
        assert torch.equal(out, _hand_loop(model, tensors, kw, want_modes))
        plain = sampling.I2VDenoiser().denoise(model, **_bf(tensors), **kw)
        assert torch.equal(plain, _hand_loop(model, tensors, kw, ["plain"] * 8))
        assert not torch.equal(out, plain)                # the feature is on
        # off in every spelling: the plain loop
        for off in (dict(attn_broadcast=None), dict(attn_broadcast=1), dict(attn_broadcast=2, attn_broadcast_range=(2.0, 3.0))):
            d2 = sampling.I2VDenoiser()
            assert torch.equal(d2.denoise(model, **off, **_bf(tensors), **kw), plain)
        # cfg_prune: a reuse step that runs more branches than the cycle's store did computes and stores
        den = sampling.I2VDenoiser()
        pruned = den.denoise(model, attn_broadcast=3, attn_broadcast_range=(0.0, 1.0), cfg_prune=True, **_bf(tensors), **kw)
        counts = den.last_branch_counts
        eff = sampling.attn_broadcast_effective(sampling.attn_broadcast_plan(ts, 3, (0.0, 1.0)), counts)
        assert den.last_attn_broadcast == eff
        assert torch.equal(pruned, _hand_loop(model, tensors, kw, eff, counts))


def test_pruned_loop_falls_back_to_a_computed_step(ab_ops, monkeypatch):
    from open_sora_amd import sampling
    from tests.test_step_cache_host import _model

    counts = [3, 1, 3, 1, 1, 3, 1, 3]
    monkeypatch.setattr(sampling, "cfg_branch_counts", lambda *a, **k: list(counts))
    cfg, tensors, kw = _case()
    model = _model(ab_ops, cfg)
    with torch.inference_mode():
        den = sampling.I2VDenoiser()
        out = den.denoise(model, attn_broadcast=3, attn_broadcast_range=(0.0, 1.0), cfg_prune=True, **_bf(tensors), **kw)
        want = ["plain", "store", "store", "reuse", "store", "store", "reuse", "plain"]
        assert den.last_attn_broadcast == want
        assert torch.equal(out, _hand_loop(model, tensors, kw, want, counts))
    calls = AB.AB_CALLS[next(iter(AB.AB_CALLS))]
    per_forward = 5                                        # depth 2 + 3 of this configuration: one copy per block (single: always; double: store only)
    stores = [c for c in calls if c[0] == "store"]
    assert [c[1] for c in stores[::per_forward]][:4] == [1, 3, 1, 3]


def test_with_the_step_cache(ab_ops):
    """a step the step cache skips launches no block: it neither stores nor reuses; threshold 0 computes every step and gives the
    attention-broadcast loop bit for bit"""
    from open_sora_amd import sampling
    from tests.test_step_cache_host import _model

    cfg, tensors, kw = _case()
    model = _model(ab_ops, cfg)
    with torch.inference_mode():
        a = sampling.I2VDenoiser().denoise(model, attn_broadcast=2, attn_broadcast_range=(0.0, 1.0), **_bf(tensors), **kw)
        den = sampling.I2VDenoiser()
        b = den.denoise(model, attn_broadcast=2, attn_broadcast_range=(0.0, 1.0), step_cache=0.0, **_bf(tensors), **kw)
        assert torch.equal(a, b) and den.last_attn_broadcast == ["plain", "store", "reuse", "store", "reuse", "store", "reuse", "plain"]
        AB.AB_CALLS.clear()
        c = den.denoise(model, attn_broadcast=2, attn_broadcast_range=(0.0, 1.0), step_cache=float("inf"), **_bf(tensors), **kw)
        assert den.last_attn_broadcast == ["plain"] + ["skipped"] * 6 + ["plain"] and not AB.AB_CALLS and torch.isfinite(c.float()).all()


# ----------------------------------------------------------------------------- keyword and environment
def test_environment_default(ab_ops, monkeypatch):
    from open_sora_amd import sampling
    from tests.test_step_cache_host import _model

    cfg, tensors, kw = _case()
    model = _model(ab_ops, cfg)
    seen = []
    monkeypatch.setattr(sampling.I2VDenoiser, "_loop_attn_broadcast", staticmethod(lambda *a: seen.append(a[-2]) or a[2]))
    monkeypatch.setattr(sampling.I2VDenoiser, "_loop", staticmethod(lambda *a: seen.append("plain") or a[2]))
    run = lambda **extra: sampling.I2VDenoiser().denoise(model, **_bf(tensors), **kw, **extra)
    ts = kw["timesteps"]
    run()
    monkeypatch.setenv("OSK_ATTN_BROADCAST", "3")
    run()
    run(attn_broadcast=None)                              # the keyword wins: off
    run(attn_broadcast=2, attn_broadcast_range=(0.0, 1.0))
    monkeypatch.setenv("OSK_ATTN_BROADCAST", " ")
    run()
    assert seen == ["plain", sampling.attn_broadcast_plan(ts, 3, (0.1, 0.8)), "plain", sampling.attn_broadcast_plan(ts, 2, (0.0, 1.0)), "plain"]
    assert sampling.ATTN_BROADCAST_RANGE == (0.1, 0.8)
    monkeypatch.setenv("OSK_ATTN_BROADCAST", "often")
    with pytest.raises(ValueError):
        run()
    monkeypatch.delenv("OSK_ATTN_BROADCAST")
    with pytest.raises(ValueError, match="attn_broadcast_range"):
        run(attn_broadcast=2, attn_broadcast_range=(0.8, 0.1))


# ----------------------------------------------------------------------------- refusals
def test_reuse_of_a_row_without_an_entry_raises(ab_ops):
    cfg, model = _tiny(ab_ops)
    a = torch_inputs(cfg, B_, T_, H_, W_, LT_, dtype=BF)
    two = {k: (v[:2] if torch.is_tensor(v) and v.shape[0] == B_ else v) for k, v in a.items()}
    with torch.inference_mode():
        ac = model.attention_broadcast_begin(B_, LT_, _LI, "cpu")
        with pytest.raises(ValueError, match="no entry"):
            model(**a, attn_cache=(ac, "reuse", (0, 1, 2)))
        model(**two, attn_cache=(ac, "store", (0, 1)))
        with pytest.raises(ValueError, match=r"\[2\]"):
            model(**a, attn_cache=(ac, "reuse", (0, 1, 2)))
        for bad in ((ac, "keep", (0, 1, 2)), (ac, "store", (0, 1)), (ac, "store", (0, 1, 1)), (ac, "store", (0, 1, 3)), (object(), "store", (0, 1, 2)), "store"):
            with pytest.raises(ValueError, match="attn_cache"):
                model(**a, attn_cache=bad)
        other = model.attention_broadcast_begin(B_, LT_ + 8, _LI, "cpu")      # another geometry replaces the set
        with pytest.raises(ValueError, match="attn_cache"):
            model(**a, attn_cache=(other, "store", (0, 1, 2)))
        assert model.attention_broadcast_begin(B_, LT_ + 8, _LI, "cpu") is other  # allocated once per key, reused
    assert other.slots.data_ptr() == model._osk_attn_cache.slots.data_ptr()


def test_refused_for_processor_calls_and_models_without_the_split(ab_ops):
    from open_sora_amd import sampling

    cfg, tensors, kw = _case()
    calls = []
    foreign = lambda **k: calls.append(1)                  # a processor-driven model: a callable without the split
    with pytest.raises(ValueError, match="split"):
        sampling.I2VDenoiser().denoise(foreign, attn_broadcast=2, **_bf(tensors), **kw)
    with pytest.raises(ValueError, match="DistilledDenoiser"):
        sampling.DistilledDenoiser().denoise(foreign, img=tensors["img"][:1], timesteps=kw["timesteps"], guidance=4.0, attn_broadcast=2)
    assert not calls
    _, model = _tiny(ab_ops)
    blk, sblk = model.double_blocks[0], model.single_blocks[0]
    x = torch.zeros(1, 8, 576, dtype=BF)
    with pytest.raises(ValueError, match="processor"):
        blk.get_processor()(blk, x, x, torch.zeros(1, 576, dtype=BF), None, attn_cache=(None, "store", (0,)))
    with pytest.raises(ValueError, match="processor"):
        sblk.get_processor()(sblk, x, torch.zeros(1, 576, dtype=BF), None, attn_cache=(None, "reuse", (0,)))


# ----------------------------------------------------------------------------- binding
def test_entry_point_is_declared_bound_and_validates_before_any_launch(hip_lib):
    with open(os.path.join(ROOT, "include", "osk.h")) as f:
        header = f.read()
    assert "int osk_attn_cache_copy_bf16(const void* src," in header and "osk_attn_cache_copy_bf16" in hip_lib.SIGNATURES
    assert "#define OSK_ABI_VERSION 2" in header and hip_lib.lib.osk_abi_version() == 2
    assert os.path.isfile(os.path.join(ROOT, "open_sora_amd", "csrc", "attn_cache.hip"))
    a, b = torch.zeros(1, 4, 16, dtype=BF), torch.zeros(1, 4, 16, dtype=BF)
    with pytest.raises(ValueError, match="osk_attn_cache_copy_bf16"):
        hip_lib.attn_cache_copy(a, b, None, True)           # CPU tensors
    f = hip_lib.lib.osk_attn_cache_copy_bf16
    assert f(None, 64, 16, 0x9000, 64, 16, None, 3, 1, 3, 4, 16, None) < 0                     # NULL view
    assert f(0x1000, 64, 16, 0x9000, 64, 16, None, 3, 1, 3, 4, 12, None) < 0                   # C % 8
    assert f(0x1008, 64, 16, 0x9000, 64, 16, None, 3, 1, 3, 4, 16, None) < 0                   # alignment
    assert f(0x1000, 64, 12, 0x9000, 64, 16, None, 3, 1, 3, 4, 16, None) < 0                   # row stride
    assert f(0x1000, 64, 16, 0x9000, 56, 16, None, 3, 1, 3, 4, 16, None) < 0                   # batch items of the slot overlap
    assert f(0x1000, 64, 16, 0x9000, 64, 16, None, 2, 1, 3, 4, 16, None) < 0                   # identity map, more items than rows
    assert f(0x1000, 64, 16, 0x9000, 64, 16, 0x5002, 3, 1, 3, 4, 16, None) < 0                 # map alignment
    assert f(0x1000, 64, 16, 0x9000, 64, 16, None, 0, 1, 3, 4, 16, None) < 0
